"""ip4_forward on the GPU (cndp_gpu_ip4_forward, include/cndp_fwd.h): fwd_edge,
arp_idx, bin_of, the counters and the WHOLE slab, byte for byte, must equal the
Python restatement (tests/fwd_ref.py) applied to the same frames, selection and
tables; a frame not taken comes back untouched.  Shapes are the smallest that
can still go wrong: one frame, a group of four and its neighbours, a wave and
its neighbours, more than one block; bursts that are no multiple of four, so
the reference's groups of four consecutive taken frames straddle lane quads,
waves and -- for n > burst -- never a burst's end."""
import os

import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.fwd import alloc_fwd_outputs

import fwd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
UDT = {"fwd_edge": np.uint16, "arp_idx": np.uint32, "bin_of": np.uint16, "stats": np.uint64}
SIZES = [1, 3, 4, 5, 63, 64, 65, 257, 1027]
BURSTS = [1, 3, 4, 5, 7, 32, 256]
SELS = ["all", "none", "second", "third", "eighth"]
LAYOUTS = ["packed", "umem", "imix"]
RX14 = 14 | 20 << 7     # l2_len 14, l3_len 20


def make_sel(kind: str, n: int) -> np.ndarray:
    s = np.zeros(n, np.uint8)
    if kind == "all":
        s[:] = 1
    elif kind == "second":
        s[::2] = 1
    elif kind == "third":
        s[::3] = 1
    elif kind == "eighth":
        s[:] = np.random.default_rng(1000 + n).random(n) < 0.125
    return s


def burst_counts(sel: np.ndarray, burst: int):
    return [int(sel[b0:b0 + burst].sum()) for b0 in range(0, len(sel), burst)]


def test_inputs_cover_tails_and_short_bursts():
    """On the CPU: the sizes x bursts x selections below hold bursts whose count
    of taken frames leaves a 1-wide tail of 1, 2 and 3, bursts with fewer than 4
    taken frames, and bursts with several groups of four."""
    tails, short, groups = set(), False, False
    for n in SIZES:
        for burst in BURSTS:
            for kind in SELS:
                for c in burst_counts(make_sel(kind, n), burst):
                    tails.add(c & 3)
                    short |= 0 < c < 4
                    groups |= c >= 8
    assert tails == {0, 1, 2, 3} and short and groups


def layout(frames, kind: str, guard: int = 0, cut: int | None = None):
    """Lay `frames` (numpy byte arrays) out: (buffer, slab_len, stride, offsets, data_off).
    guard bytes of 0xA5 follow the slab; cut = bytes of the last frame inside the slab."""
    n = len(frames)
    if kind == "packed":
        stride, data_off, offs = 64, 0, None
        starts = [i * 64 for i in range(n)]
        total = n * 64
    elif kind == "umem":
        stride, data_off, offs = 2048, 256, None
        starts = [i * 2048 + 256 for i in range(n)]
        total = n * 2048
    else:       # IMIX: 64 / 570 / 1500-byte slots at 7:4:1, packed at roundup(len, 64)
        pick = np.random.default_rng(n).integers(0, 12, n)
        slot = np.where(pick < 7, 64, np.where(pick < 11, 576, 1536))
        offs = (np.cumsum(slot) - slot).astype(np.int64)
        stride, data_off = 0, 0
        starts = offs.tolist()
        total = int(slot.sum())
    slab_len = total if cut is None else starts[-1] + cut
    buf = np.zeros(max(total, slab_len) + guard, np.uint8)
    for s, f in zip(starts, frames):
        buf[s:s + len(f)] = f
    buf[slab_len:] = 0xA5
    return buf, slab_len, stride, offs, data_off


def host(t, dt):
    return t.cpu().numpy().view(dt)


def run(cl, tbl, w, lay, n, gpu, burst=256, sel=None, rxmeta=None, nh=None, ptype=None, n_bins=8, slab_t=None,
        want_slab=None, stats0=None, fwd=None, stream=None):
    """One call of the stage against the restatement; returns (got, want, slab tensor, expected slab)."""
    buf, slab_len, stride, offs, data_off = lay
    if slab_t is None:
        slab_t = torch.from_numpy(buf.copy()).to(gpu)
        want_slab = buf.copy()
    offs_t = torch.from_numpy(offs).to(gpu) if offs is not None else None
    fr = pktgen.Frames(slab_t[:slab_len], n, stride=stride, offsets=offs_t, data_off=data_off)
    rxmeta = np.full(n, RX14, np.uint32) if rxmeta is None else np.asarray(rxmeta, np.uint32)
    nh = np.full(n, 1 << 24, np.uint32) if nh is None else np.asarray(nh, np.uint32)
    out = {"nh": torch.from_numpy(nh.view(np.int32)).to(gpu), "rxmeta": torch.from_numpy(rxmeta.view(np.int32)).to(gpu)}
    if ptype is not None:
        out["ptype"] = torch.from_numpy(np.asarray(ptype, np.uint32).view(np.int32)).to(gpu)
    sel_t = torch.from_numpy(np.ascontiguousarray(sel, np.uint8)).to(gpu) if sel is not None else None
    if stream is not None:
        torch.cuda.synchronize()        # the inputs above were made on the current stream
    got_t = cl.ip4_forward(fr, out, tbl, burst=burst, sel=sel_t, n_bins=n_bins, fwd=fwd, stream=stream)
    torch.cuda.synchronize()
    got = {k: host(got_t[k], dt) for k, dt in UDT.items()}
    want = R.ip4_forward_ref(want_slab, n, rxmeta, burst, w, sel=sel, nh=nh, ptype=ptype, stride=stride,
                             offsets=offs, data_off=data_off, n_bins=n_bins, stats=stats0, slab_len=slab_len)
    what = f"burst {burst}"
    for k in UDT:
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, (f"{what}: {k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]:#x} "
                               f"want {want[k][bad[0]]:#x}")
    got_slab = slab_t.cpu().numpy()
    bad = np.nonzero(got_slab != want_slab)[0]
    assert len(bad) == 0, (f"{what}: slab: {len(bad)} bytes differ, first at {bad[0]} (slab_len {slab_len}): "
                           f"got {got_slab[bad[0]]:#x} want {want_slab[bad[0]]:#x}")
    got["fwd"] = got_t
    return got, want, slab_t, want_slab


def pool_frames(n, seed, pool=None, l2=(14,)):
    rng = np.random.default_rng(seed)
    pool = pool or R.DST_POOL
    return [R.ip4_frame(pool[int(rng.integers(0, len(pool)))], ttl=int(rng.integers(0, 256)),
                        l2=int(l2[int(rng.integers(0, len(l2)))])) for _ in range(n)]


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def std(gpu):
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    yield w, tbl
    R.close_tables(arp, rt4, tbl)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_layouts_bursts(cl, std, gpu, n, kind):
    w, tbl = std
    lay = layout(pool_frames(n, n), kind, guard=64)
    kinds = np.zeros(3, np.uint64)
    for burst in BURSTS:
        for sk in SELS:
            sel = make_sel(sk, n)
            got, want, _, _ = run(cl, tbl, w, lay, n, gpu, burst=burst, sel=sel)
            assert ((got["fwd_edge"] != 0xFFFF) == (sel != 0)).all()
            kinds += want["stats"]
    if n >= 63:
        assert kinds.all()      # direct, via a gateway and arp_request all occur


def _burst(dsts, taken, size=8):
    """A burst of `size` frames whose first len(dsts) taken positions carry dsts."""
    assert len(dsts) == len(taken) and max(taken) < size
    frames = [R.ip4_frame("192.0.2.9") for _ in range(size)]
    sel = np.zeros(size, np.uint8)
    for d, p in zip(dsts, taken):
        frames[p] = R.ip4_frame(d)
        sel[p] = 1
    return frames, sel


@pytest.mark.gpu
def test_group_rules(cl, std, gpu):
    """Hand-built bursts of 4, 5, 8 and 7 taken frames (burst 8, frames not
    taken between them), each group's outcome spelt out."""
    w, tbl = std
    D, G1, G2, G4, G6 = "10.1.0.2", "10.2.0.5", "10.3.1.1", "10.8.3.3", "10.10.1.1"
    X, NR, U = "10.4.1.1", "192.0.2.1", "10.5.1.1"
    bursts = [
        _burst([D, G1, G2, G4], [0, 2, 5, 7]),                              # A: 4 taken
        _burst([D, G1, G2, G4, G1], [1, 2, 3, 4, 6]),                       # B: 5 taken: a group and a tail
        _burst([G1, G2, G4, G6, X, NR, G2, U], list(range(8))),             # C: 8 taken: two groups
        _burst([NR, NR, NR, NR, G1, G2, G4], [0, 1, 2, 3, 4, 5, 7]),        # D: 7 taken: a group, a tail of 3
        _burst([G1, NR, G2, G4, NR, NR, "10.7.0.1", "10.7.0.2"], list(range(8))),   # E
    ]
    frames = [f for b in bursts for f in b[0]]
    sel = np.concatenate([b[1] for b in bursts])
    n = len(frames)
    for kind in ("packed", "imix"):
        got, want, _, _ = run(cl, tbl, w, layout(frames, kind), n, gpu, burst=8, sel=sel)
    e, a = want["fwd_edge"], want["arp_idx"]
    NONE = N.CNDP_FWD_NONE

    def at(b, k):
        return b * 8 + int(np.nonzero(bursts[b][1])[0][k])

    # A: one direct hit: the three with route + gateway go to arp_request
    assert [int(e[at(0, k)]) for k in range(4)] == [1 + 2, 1, 1, 1] and a[at(0, 0)] == 2
    assert all(a[at(0, k)] == NONE for k in (1, 2, 3))
    # B: the same, and the tail frame is transmitted via its gateway
    assert int(e[at(1, 4)]) == 2 + 2 and a[at(1, 4)] == 1 and int(e[at(1, 1)]) == 1
    # D: the same three in a tail position: via their own gateways
    assert [int(e[at(3, k)]) for k in (4, 5, 6)] == [2 + 2, 3 + 2, 4 + 2]
    assert [int(a[at(3, k)]) for k in (4, 5, 6)] == [1, 12, 14]
    # C, first group: four gateways: lanes 1-3 carry gateway 0's ha, their own route's netif
    assert [int(e[at(2, k)]) for k in range(4)] == [2 + 2, 3 + 2, 4 + 2, 0 + 2]
    assert [int(a[at(2, k)]) for k in range(4)] == [1, 1, 1, 1]
    # C, second group: lane 0's gateway has no entry, lane 2's has: its own ha
    assert [int(e[at(2, k)]) for k in range(4, 8)] == [1, 1, 3 + 2, 1] and a[at(2, 6)] == 12
    # E, first group: a member with no route; second: no member with a route
    assert [int(e[at(4, k)]) for k in range(4)] == [2 + 2, 1, 3 + 2, 4 + 2]
    assert [int(a[at(4, k)]) for k in range(4)] == [1, NONE, 1, 1]
    assert [int(e[at(4, k)]) for k in range(4, 8)] == [1, 1, 1, 1]
    # the quirk on the wire: lane 2 of C's first group has gateway 0's MAC as d_addr
    lay = layout(frames, "packed")
    _, _, slab_t, _ = run(cl, tbl, w, lay, n, gpu, burst=8, sel=sel)
    f = slab_t.cpu().numpy()[at(2, 2) * 64:][:12]
    assert bytes(f[:6]) == w.arp[1][1] and bytes(f[6:]) == w.netif[4]


@pytest.mark.gpu
def test_checksum_and_ttl_golden(cl, std, gpu):
    """The reference's recorded (ttl, checksum) results as frames through the kernel."""
    w, tbl = std
    g = np.load(os.path.join(HERE, "golden", "ip4_fwd_cksum_ref.npz"))
    n = len(g["ttl"])
    rng = np.random.default_rng(5)
    frames = [R.ip4_frame(R.DST_POOL[int(rng.integers(0, len(R.DST_POOL)))], ttl=int(t), ck=int(c))
              for t, c in zip(g["ttl"], g["cksum"])]
    lay = layout(frames, "packed")
    _, _, slab_t, _ = run(cl, tbl, w, lay, n, gpu, burst=256, sel=np.ones(n, np.uint8))
    rows = slab_t.cpu().numpy().reshape(n, 64)
    assert np.array_equal(rows[:, 22], g["ttl_out"])
    assert np.array_equal(rows[:, 24].astype(np.uint16) | rows[:, 25].astype(np.uint16) << 8, g["cksum_out"])


@pytest.mark.gpu
def test_l2_len(cl, std, gpu):
    """VLAN (18) and QinQ (22) frames: the MACs land at the frame start, TTL and
    checksum at l2_len + 8 / + 10."""
    w, tbl = std
    n = 67
    l2 = np.array([(14, 18, 22)[(i + i // 15) % 3] for i in range(n)])   # every l2_len in a burst's tail too
    frames = [R.ip4_frame("10.1.0.2" if i % 3 else "10.3.1.1", ttl=9, l2=int(l2[i])) for i in range(n)]
    rx = (l2 | 20 << 7).astype(np.uint32)
    for kind in ("packed", "umem"):
        lay = layout(frames, kind)
        _, want, slab_t, _ = run(cl, tbl, w, lay, n, gpu, burst=5, sel=np.ones(n, np.uint8), rxmeta=rx)
    rows = slab_t.cpu().numpy().reshape(n, 2048)[:, 256:]
    macs = set()
    for i in range(n):
        assert rows[i, int(l2[i]) + 8] == 8
        assert rows[i, 12] in (0x08, 0x81, 0x88)        # the tags are where they were
        if want["fwd_edge"][i] != 1:
            macs.add((int(l2[i]), bytes(rows[i, 6:12])))
        else:
            assert bytes(rows[i, :12]) == bytes.fromhex("0200000000010200000000ff")
    # direct and (in the bursts' 1-wide tails) via a gateway, at every l2_len
    assert macs == {(l, m) for l in (14, 18, 22) for m in (w.netif[1], w.netif[3])}


@pytest.mark.gpu
def test_slab_end(cl, gpu):
    """The last frame's header straddles slab_len: bytes past it read as zero
    (a destination cut to 0.0.0.0 is given an ARP entry of its own, so the MAC
    stores are attempted too) and nothing at or past slab_len is written -- the
    guard bytes after the slab come back as they were."""
    w = R.standard_world()
    w.arp_fib.add(0, 32, 2)
    arp, rt4, tbl = R.make_tables(w)
    try:
        frames = pool_frames(4, 3) + [R.ip4_frame("10.1.0.3", ttl=1)]
        for kind in ("packed", "imix"):
            for cut in (1, 3, 6, 7, 11, 12, 13, 22, 23, 24, 25, 26, 30, 31, 33, 34, 60):
                lay = layout(frames, kind, guard=96, cut=cut)
                for burst in (4, 256):
                    got, want, slab_t, _ = run(cl, tbl, w, lay, 5, gpu, burst=burst, sel=np.ones(5, np.uint8))
                    assert (slab_t.cpu().numpy()[lay[1]:] == 0xA5).all()
                    if cut <= 30:
                        assert want["arp_idx"][4] == 2      # dst read as 0.0.0.0 (or cut short of it)
    finally:
        R.close_tables(arp, rt4, tbl)


def classify(cl, fr):
    cl.set_tuning(cnet_spec=256)    # a fresh ptype-node state
    out = cl.alloc_outputs(fr.n, 64, device=fr.slab.device, meta=True)
    cl.classify(fr, N.CNDP_MODE_CNET, out=out)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def cnet_world(gpu, cl):
    """The C4 batch (IMIX sizes, IPv4 / IPv6, cnet routes) classified, and a
    world whose FIBs cover its IPv4 destinations (10.0.0.0/14)."""
    from helpers import cnet_fibs
    fib, fib6, routes, v6, _, _ = cnet_fibs()
    cl.set_fib(fib, fib6)
    w = R.standard_world()
    w.arp[4] = (3, w.arp[4][1])
    w.arp_fib.add(R.ip_h("10.0.0.0"), 16, 4)        # 10.0/16 directly attached
    arp, rt4, tbl = R.make_tables(w)
    n = 1027
    fr = pktgen.imix(n, seed=21, v4routes=routes, v6routes=v6, device=gpu)
    out = classify(cl, fr)
    yield w, tbl, fr, out
    R.close_tables(arp, rt4, tbl)
    fib.close()
    fib6.close()


def _lay_of(fr):
    buf = fr.slab.cpu().numpy().copy()
    return buf, len(buf), fr.stride, fr.offsets.cpu().numpy(), fr.data_off


@pytest.mark.gpu
def test_selection(cl, cnet_world, gpu):
    """Derived selection against the same selection given explicitly; frames on
    ip4_input's proto and drop edges and IPv6 frames are never taken."""
    w, tbl, fr, out = cnet_world
    n = fr.n
    nh, pt, rx = host(out["nh"], np.uint32), host(out["ptype"], np.uint32), host(out["rxmeta"], np.uint32)
    lay = _lay_of(fr)
    got_d, want_d, _, _ = run(cl, tbl, w, lay, n, gpu, burst=256, nh=nh, ptype=pt, rxmeta=rx)
    taken = got_d["fwd_edge"] != 0xFFFF
    is4 = np.isin(pt & 0xFFFF, R.IP4_INPUT_TYPES)
    edge = np.where(nh == N.CNDP_NH_INVALID, 0xFF, nh >> 24)
    assert np.array_equal(taken, is4 & (edge == 1))
    assert taken.sum() > 100 and (is4 & (edge == 2)).sum() > 0 and (is4 & (edge == 0)).sum() > 5
    from helpers import ptype_ref
    C = ptype_ref()["ptype_consts"]
    is6 = (pt & C["CNE_PTYPE_L3_MASK"]) == C["CNE_PTYPE_L3_IPV6"]
    assert is6.sum() > 100 and not taken[is6].any()
    assert want_d["stats"].all()
    got_s, _, _, _ = run(cl, tbl, w, lay, n, gpu, burst=256, sel=taken.astype(np.uint8), nh=nh, ptype=pt, rxmeta=rx)
    for k in UDT:
        assert np.array_equal(got_s[k], got_d[k]), k
    # no frame taken: every output "none", the counters as they were
    fwd = alloc_fwd_outputs(n, gpu)
    fwd["stats"] += torch.tensor([5, 6, 7], dtype=torch.int64, device=gpu)
    got, _, _, _ = run(cl, tbl, w, lay, n, gpu, burst=32, sel=np.zeros(n, np.uint8), rxmeta=rx, fwd=fwd,
                       stats0=[5, 6, 7])
    assert (got["fwd_edge"] == 0xFFFF).all() and got["stats"].tolist() == [5, 6, 7]


@pytest.mark.gpu
def test_table_changes_between_calls(cl, gpu):
    """Object set / clear, a netif MAC, an ARP /32 and a route added and deleted
    (the FIB mirrors' paint), each followed by a call that must see it."""
    w = R.standard_world()
    arp, rt4, tbl = R.make_tables(w)
    try:
        n = 257
        pool = R.DST_POOL + ["10.1.0.77", "10.2.200.9"]
        lay = layout(pool_frames(n, 17, pool=pool), "packed")
        sel = np.ones(n, np.uint8)

        def first(dst, tail=False):
            # tail: a position the burst of 7 handles 1-wide, where a route's gateway
            # is used whatever the frame's neighbours hit
            return next(i for i in range(n) if bytes(lay[0][i * 64 + 30:i * 64 + 34]) == bytes(dst)
                        and (not tail or i % 7 >= 4))

        i77, i200, i2 = first([10, 1, 0, 77]), first([10, 2, 200, 9], tail=True), first([10, 1, 0, 2])

        def call():
            return run(cl, tbl, w, lay, n, gpu, burst=7, sel=sel)[1]

        want = call()
        assert want["fwd_edge"][i77] == 1 and want["fwd_edge"][i200] == 2 + 2
        ha = bytes([2, 0xDD, 1, 2, 3, 4])
        assert tbl.arp_set(2, 5, ha) == 0                   # an object replaced
        w.arp[2] = (5, ha)
        assert call()["fwd_edge"][i2] == 5 + 2
        assert tbl.arp_clear(2) == 0                        # ... and cleared
        del w.arp[2]
        assert call()["arp_idx"][i2] != 2
        mac = bytes([2, 0x77, 0, 0, 0, 1])
        assert tbl.netif_set(2, mac) == 0                   # a netif's MAC
        w.netif[2] = mac
        call()
        assert arp.add(R.ip_h("10.1.0.77"), 32, 6) == 0     # an ARP /32 added
        w.arp_fib.add(R.ip_h("10.1.0.77"), 32, 6)
        want = call()
        assert want["fwd_edge"][i77] == 5 + 2 and want["arp_idx"][i77] == 6
        assert arp.delete(R.ip_h("10.1.0.77"), 32) == 0     # ... and deleted
        w.arp_fib.delete(R.ip_h("10.1.0.77"), 32)
        assert call()["fwd_edge"][i77] == 1
        assert rt4.add(R.ip_h("10.2.200.0"), 24, 2) == 0    # a more specific route
        w.rt_fib.add(R.ip_h("10.2.200.0"), 24, 2)
        want = call()
        assert want["fwd_edge"][i200] == 3 + 2 and want["arp_idx"][i200] == 12
        assert rt4.delete(R.ip_h("10.2.200.0"), 24) == 0
        w.rt_fib.delete(R.ip_h("10.2.200.0"), 24)
        assert tbl.rt_clear(1) == 0                         # a route object cleared
        del w.rt[1]
        want = call()
        assert want["fwd_edge"][i200] == 1
        assert tbl.rt_set(1, R.ip_h("10.9.0.4"), 0) == 0    # ... and set again, elsewhere
        w.rt[1] = (R.ip_h("10.9.0.4"), 0)
        call()
    finally:
        R.close_tables(arp, rt4, tbl)


@pytest.mark.gpu
def test_streams(cl, std, gpu):
    """A call on a second stream after one on the first, on the same slab: the
    second starts from the first's result (TTL and checksum stepped twice)."""
    w, tbl = std
    n = 1027
    lay = layout(pool_frames(n, 23), "packed")
    sel = make_sel("second", n)
    s1, s2 = torch.cuda.Stream(device=gpu), torch.cuda.Stream(device=gpu)
    _, _, slab_t, want_slab = run(cl, tbl, w, lay, n, gpu, burst=32, sel=sel, stream=s1.cuda_stream)
    _, _, slab_t, want_slab = run(cl, tbl, w, lay, n, gpu, burst=32, sel=sel, stream=s2.cuda_stream, slab_t=slab_t,
                                  want_slab=want_slab)
    # without a host wait between them
    slab_t = torch.from_numpy(lay[0].copy()).to(gpu)
    fr = pktgen.Frames(slab_t, n, stride=64)
    out = {"nh": torch.full((n,), 1 << 24, dtype=torch.int32, device=gpu),
           "rxmeta": torch.full((n,), RX14, dtype=torch.int32, device=gpu)}
    sel_t = torch.from_numpy(sel).to(gpu)
    fwd = alloc_fwd_outputs(n, gpu)
    torch.cuda.synchronize()
    for s in (s1, s2, s1, s2):
        cl.ip4_forward(fr, out, tbl, burst=32, sel=sel_t, stream=s.cuda_stream, fwd=fwd)
    torch.cuda.synchronize()
    ref = lay[0].copy()
    for _ in range(4):
        R.ip4_forward_ref(ref, n, np.full(n, RX14, np.uint32), 32, w, sel=sel, stride=64)
    assert np.array_equal(slab_t.cpu().numpy(), ref)


@pytest.mark.gpu
def test_chain_classify_forward_partition(cl, cnet_world, gpu):
    """cnet classify -> ip4_forward -> cndp_gpu_bin_partition at n_bins = 8:
    every netif's transmit list is its frames' indices in arrival order."""
    w, tbl, fr, out = cnet_world
    n = fr.n
    nh, pt, rx = host(out["nh"], np.uint32), host(out["ptype"], np.uint32), host(out["rxmeta"], np.uint32)
    assert tbl.max_netif() == 7
    got, want, _, _ = run(cl, tbl, w, _lay_of(fr), n, gpu, burst=256, nh=nh, ptype=pt, rxmeta=rx, n_bins=8)
    start, order = cl.bin_partition(got["fwd"]["bin_of"], 8)
    torch.cuda.synchronize()
    start, order, bins = host(start, np.uint32), host(order, np.uint32), got["bin_of"]
    assert start[0] == 0 and start[8 + 2] == n
    used = 0
    for b in range(8 + 2):
        idx = np.nonzero(bins == b)[0]
        assert np.array_equal(order[start[b]:start[b + 1]], idx), b
        used += b < 8 and len(idx) > 0
    assert used >= 2 and (bins == 8).any() and (bins == 9).any()
    with pytest.raises(OSError) as e:       # n_bins must exceed the largest netif the table holds
        run(cl, tbl, w, _lay_of(fr), n, gpu, burst=256, nh=nh, ptype=pt, rxmeta=rx, n_bins=7)
    assert e.value.errno == 22


@pytest.mark.gpu
def test_arguments(cl, std, gpu):
    w, tbl = std
    n = 5
    lay = layout(pool_frames(n, 1), "packed")
    slab_t = torch.from_numpy(lay[0].copy()).to(gpu)
    fr = pktgen.Frames(slab_t, n, stride=64)
    full = {"nh": torch.full((n,), 1 << 24, dtype=torch.int32, device=gpu),
            "rxmeta": torch.full((n,), RX14, dtype=torch.int32, device=gpu)}
    sel_t = torch.ones(n, dtype=torch.uint8, device=gpu)

    def refused(out=full, burst=256, sel=sel_t, fwd=None):
        with pytest.raises(OSError) as e:
            cl.ip4_forward(fr, out, tbl, burst=burst, sel=sel, fwd=fwd)
        return e.value.errno == 22

    assert refused(burst=0) and refused(burst=257)
    assert refused(out={"rxmeta": full["rxmeta"]}) and refused(out={"nh": full["nh"]})
    assert refused(fwd=alloc_fwd_outputs(n, gpu) | {"fwd_edge": None})
    assert refused(sel=None)            # derived selection without ptype
    torch.cuda.synchronize()
    assert np.array_equal(slab_t.cpu().numpy(), lay[0])     # a refused call touches nothing
    cl.ip4_forward(fr, full, tbl, burst=1, sel=sel_t)       # the ends of the range run
    cl.ip4_forward(fr, full, tbl, burst=256, sel=sel_t)
    empty = pktgen.Frames(slab_t, 0, stride=64)
    cl.ip4_forward(empty, full, tbl, burst=256, sel=sel_t)  # an empty batch is no error
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_table_is_bound_to_one_device(std, gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: a table used on cuda:0 must refuse a call on cuda:1")
    from cndp_amd.classify import Classifier
    w, tbl = std
    c0, c1 = Classifier(0), Classifier(1)
    try:
        for c, dev, ok in ((c0, "cuda:0", True), (c1, "cuda:1", False)):
            lay = layout(pool_frames(5, 1), "packed")
            slab_t = torch.from_numpy(lay[0].copy()).to(dev)
            fr = pktgen.Frames(slab_t, 5, stride=64)
            out = {"nh": torch.full((5,), 1 << 24, dtype=torch.int32, device=dev),
                   "rxmeta": torch.full((5,), RX14, dtype=torch.int32, device=dev)}
            sel_t = torch.ones(5, dtype=torch.uint8, device=dev)
            if ok:
                c.ip4_forward(fr, out, tbl, sel=sel_t)
            else:
                with pytest.raises(OSError) as e:
                    c.ip4_forward(fr, out, tbl, sel=sel_t)
                assert e.value.errno == 22
    finally:
        c0.close()
        c1.close()

"""cndpfwd's fwd and l3fwd modes on the host (include/cndp_cfwd.h,
cndp_amd/csrc/cfwd.c): the restatement (tests/cfwd_ref.py) against what the
reference's compiled FIB and cne_inet4.h recorded in
tests/golden/cndpfwd_l3_ref.npz, the host rule (cndp_cfwd_host) against both --
outputs, counters and the whole slab, byte for byte -- the checksum step against
tests/golden/ip4_fwd_cksum_ref.npz (main.c:225-237 is the text of
cnet_ipv4.h:159-170), the helpers' packing and refusals, the argument checks,
and cfwd.c under the address and undefined-behaviour sanitizers in a
stand-alone program.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.cfwd import cfwd_host, l3fwd_fib, nexthop, route_add, route_add_raw
from cndp_amd.fib import Fib

import cfwd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("nh", "tx_lport", "echoed", "bin_of", "stats")


@pytest.fixture(scope="module")
def fib():
    f = R.apply_ops(l3fwd_fib())
    yield f
    f.close()


@pytest.fixture(scope="module")
def routes():
    return R.routes_of(R.golden())


def same(got: dict, want: dict, buf=None):
    for k in KEYS:
        bad = np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]} want {want[k][bad[0]]}"
    if buf is not None:
        bad = np.nonzero(buf != want["slab"])[0]
        assert len(bad) == 0, f"slab: {len(bad)} bytes differ, first at {bad[0]}"


def test_golden_file_meets_its_conditions():
    g = R.golden()
    assert os.path.getsize(os.path.join(HERE, "golden", "cndpfwd_l3_ref.npz")) < 65536
    adds = g["op_del"] == 0
    assert 250 <= np.count_nonzero(adds) <= 350 and np.count_nonzero(~adds) >= 20
    assert set(np.unique(g["op_depth"][adds])) == {1, 8, 9, 16, 23, 24, 25, 31, 32}
    assert set(np.unique(g["op_port"][adds])) == {0, 1, 7, 255, 256, 0x7FFF}
    assert len(g["addr"]) == 2048
    miss = g["nh"] == R.DEFAULT_NH
    assert 100 < np.count_nonzero(miss) < 1024 and set(np.unique(g["tx_port"])) == {0, 1, 7, 255, 256, 0x7FFF}
    # prefixes nest: some address is covered by three routes or more, and some by a /25 or longer
    rt = R.routes_of(g)
    cover = np.zeros(2048, int)
    deep = np.zeros(2048, bool)
    for (prefix, depth), _ in rt.items():
        hit = (g["addr"].astype(np.int64) & R.mask(depth)) == prefix
        cover += hit
        deep |= hit & (depth > 24)
    assert cover.max() >= 3 and deep.any()
    # a deleted route's addresses fall back to a parent in force, or miss
    gone = [(ip & R.mask(d), d) for ip, d, dele in zip(g["op_ip"].tolist(), g["op_depth"].tolist(), g["op_del"].tolist()) if dele]
    fell = [np.count_nonzero(((g["addr"].astype(np.int64) & R.mask(d)) == p)) for p, d in gone if (p, d) not in rt]
    assert sum(fell) > 0


def test_restatement_equals_the_recorded_results(routes):
    g = R.golden()
    nh = R.lookup(routes, g["addr"])
    bad = np.nonzero(nh != g["nh"])[0]
    assert len(bad) == 0, f"{len(bad)} of 2048 differ, first at {bad[0]}: {nh[bad[0]]:#x} != {g['nh'][bad[0]]:#x}"
    assert np.array_equal(R.h64tom(nh), g["mac"])                                   # inet_h64tom
    assert np.array_equal((nh >> np.uint64(48)).astype(np.uint16), g["tx_port"])    # l3-fwd.c:89
    for mac, port in zip(g["op_mac"][:32], g["op_port"][:32].tolist()):             # inet_mtoh64 and :67, both ways
        v = R.nexthop(mac, port)
        assert np.array_equal(R.h64tom([v])[0], mac) and v >> 48 == port


def test_fib_image_equals_the_recorded_results(fib):
    g = R.golden()
    assert np.array_equal(fib.lookup_bulk(g["addr"]), g["nh"])


@pytest.mark.parametrize("kind", ("packed", "umem", "offsets"))
@pytest.mark.parametrize("mode", (R.FWD, R.L3FWD))
def test_host_rule_equals_the_restatement_and_the_golden(fib, routes, mode, kind):
    g = R.golden()
    rows = R.frames(g["addr"], dmac5=np.arange(2048) % 9, ttl=np.arange(2048) % 256, seed=5)
    slab, lay = R.layout(rows, kind)
    for lports, in_lport in (((0, 1, 7, 255), 3), ((1, 7), 1)):      # with port 0, and without: a miss is echoed
        buf = slab.copy()
        kw = dict(in_lport=in_lport, lports=lports, **lay)
        got = cfwd_host(buf, 2048, mode, fib=fib, **kw)
        want = R.cfwd_ref(slab, 2048, mode, routes=routes, **kw)
        same(got, want, buf)
        if mode == R.L3FWD:
            assert np.array_equal(got["nh"], g["nh"]), "differs from the next hops the reference recorded"
            at = R.frame_starts(2048, **lay)
            rew = got["echoed"] == 0
            assert np.array_equal(np.stack([buf[at + k] for k in range(6)], 1)[rew], g["mac"][rew])
            assert np.array_equal(got["tx_lport"][rew], g["tx_port"][rew])
            assert set(g["tx_port"][~rew].tolist()) == ({256, 0x7FFF} if 0 in lports else {0, 255, 256, 0x7FFF})
        else:
            assert not got["nh"].any()


def test_checksum_step_equals_the_reference_golden(fib):
    g = np.load(os.path.join(HERE, "golden", "ip4_fwd_cksum_ref.npz"))
    n = len(g["ttl"])
    rows = R.frames(np.zeros(n, np.uint32), ttl=g["ttl"], ck=g["cksum"])
    buf = rows.reshape(-1).copy()
    cfwd_host(buf, n, R.L3FWD, fib=fib, lports=(0,), stride=64)
    out = buf.reshape(n, 64)
    assert np.array_equal(out[:, 22], g["ttl_out"])
    assert np.array_equal(out[:, 24].astype(np.uint16) | out[:, 25].astype(np.uint16) << 8, g["cksum_out"])
    assert np.array_equal(R.adjust_cksum(g["cksum"]), g["cksum_out"])
    pairs = set(zip(g["ttl"].tolist(), g["cksum"].tolist()))
    assert pairs >= {(t, c) for t in (0, 1) for c in (0x0000, 0xFFFF, 0xFEFF, 0xFF00)}


def test_quirks_kept(fib, routes):
    """An ARP frame and one whose byte 14 is not 0x45 are edited like any other;
    a miss goes out of port 0 as a broadcast; the source MAC survives MAC_REWRITE."""
    g = R.golden()
    hit = int(np.nonzero(g["tx_port"] == 1)[0][0])
    miss = int(np.nonzero(g["nh"] == R.DEFAULT_NH)[0][0])
    rows = R.frames(g["addr"][[hit, hit, miss, hit]], ttl=[64, 0, 1, 9], ck=[0x1234, 0, 0xFFFF, 0xFEFF])
    rows[0, 12:14] = (0x08, 0x06)
    rows[1, 14] = 0x60
    buf = rows.reshape(-1).copy()
    got = cfwd_host(buf, 4, R.L3FWD, fib=fib, in_lport=2, lports=(0, 1, 2), stride=64)
    same(got, R.cfwd_ref(rows.reshape(-1), 4, R.L3FWD, routes=routes, in_lport=2, lports=(0, 1, 2), stride=64), buf)
    out = buf.reshape(4, 64)
    assert out[:, 22].tolist() == [63, 255, 0, 8] and got["tx_lport"].tolist() == [1, 1, 0, 1]
    assert out[2, :6].tolist() == [255] * 6 and np.array_equal(out[:, 6:12], rows[:, 6:12])
    assert np.array_equal(out[0, :6], g["mac"][hit]) and got["stats"].tolist() == [4, 0]


def test_slab_edge_selection_and_counters(fib, routes):
    g = R.golden()
    n = 65
    rows = R.frames(g["addr"][:n], dmac5=np.arange(n) % 4, seed=9)
    stats = None
    for kind in ("packed", "offsets"):
        slab, lay = R.layout(rows, kind)
        last = int(R.frame_starts(n, **lay)[-1])
        for mode in (R.FWD, R.L3FWD):
            for cut in (5, 11, 22, 24, 33, 0):
                for sel in (None, np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), (np.arange(n) % 2 == 0).astype(np.uint8)):
                    buf = slab.copy()
                    kw = dict(in_lport=1, lports=(0, 1, 2), sel=sel, slab_len=last + cut, **lay)
                    got = cfwd_host(buf, n, mode, fib=fib, stats=stats, **kw)
                    want = R.cfwd_ref(slab, n, mode, routes=routes, stats=stats, **kw)
                    same(got, want, buf)
                    assert np.array_equal(buf[last + cut:], slab[last + cut:])
                    stats = got["stats"]
                    if sel is not None:
                        off = sel == 0
                        assert (got["tx_lport"][off] == 0xFFFF).all() and (got["bin_of"][off] == 3).all() and not got["nh"][off].any()
    assert stats.sum() > 0


def test_helpers_pack_and_refuse():
    L = N.lib()
    assert nexthop("02:aa:bb:cc:dd:ee", 7) == 0x000702AABBCCDDEE == R.nexthop(bytes.fromhex("02aabbccddee"), 7)
    assert nexthop(bytes(6), 0xFFFF) == 0xFFFF << 48 and L.cndp_cfwd_nexthop(None, 1) == 0
    assert not L.cndp_cfwd_fib_create(None)
    fib = l3fwd_fib("x")
    assert fib.lookup_bulk([0, 0xFFFFFFFF]).tolist() == [R.DEFAULT_NH] * 2        # l3-fwd.c:100
    mac = bytes.fromhex("02aabbccddee")
    assert route_add_raw(fib, 0x0A000000, 8, mac, 0x8000) == -22 and route_add_raw(fib, 0x0A000000, 8, mac, 0xFFFF) == -22
    assert route_add_raw(fib, 0x0A000000, 33, mac, 1) == -22
    assert L.cndp_cfwd_route_add(None, 0, 8, mac, 1) == -22 and L.cndp_cfwd_route_add(fib.h, 0, 8, None, 1) == -22
    assert fib.lookup_bulk([0x0A000001]).tolist() == [R.DEFAULT_NH]               # nothing was added
    route_add(fib, 0x0A000000, 8, mac, 0x7FFF)
    assert fib.lookup_bulk([0x0A000001]).tolist() == [0x7FFF02AABBCCDDEE]         # the highest port round-trips
    for i in range(300):                                                          # /32s behind one /24: tbl8 groups
        route_add(fib, 0x0B000000 + 256 * (i // 2) + i, 32, mac, i % 8)
    assert fib.lookup_bulk([0x0B000000 + 256 * 149 + 299]).tolist() == [(299 % 8) << 48 | 0x02AABBCCDDEE]
    fib.close()


def test_argument_checks_and_n_zero(fib):
    L = N.lib()
    rows = R.frames(np.array([0x01020304], np.uint32))
    orig = rows.copy()
    f4 = Fib("narrow", N.CNE_FIB_DIR24_8, default_nh=0, max_routes=16, nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=16)
    rc, r = cfwd_host(rows.reshape(-1), 1, R.L3FWD, fib=f4, lports=(0,), stride=64, raw=True)
    assert rc == -22 and np.array_equal(rows, orig) and not r["stats"].any()      # 4-byte entries: refused
    f4.close()
    rc, _ = cfwd_host(rows.reshape(-1), 1, R.L3FWD, fib=None, lports=(0,), stride=64, raw=True)
    assert rc == -22                                                               # L3FWD needs a FIB
    rc, _ = cfwd_host(rows.reshape(-1), 1, 2, fib=fib, lports=(0,), stride=64, raw=True)
    assert rc == -22                                                               # unknown mode
    b, io = N.Batch(), N.CfwdIo()
    tx = np.zeros(1, np.uint16)
    b.n, b.slab, b.slab_len, b.stride = 1, rows.ctypes.data, rows.size, 64
    io.tx_lport = tx.ctypes.data
    assert L.cndp_cfwd_host(fib.h, None, 1, ctypes.byref(io)) == -22 and L.cndp_cfwd_host(fib.h, ctypes.byref(b), 1, None) == -22
    io.tx_lport = None
    assert L.cndp_cfwd_host(fib.h, ctypes.byref(b), 1, ctypes.byref(io)) == -22
    io.tx_lport, io.in_lport = tx.ctypes.data, 256
    assert L.cndp_cfwd_host(fib.h, ctypes.byref(b), 1, ctypes.byref(io)) == -22
    io.in_lport, b.slab = 0, None
    assert L.cndp_cfwd_host(fib.h, ctypes.byref(b), 1, ctypes.byref(io)) == -22
    b.slab, b.slab_len = rows.ctypes.data, 1 << 63
    assert L.cndp_cfwd_host(fib.h, ctypes.byref(b), 1, ctypes.byref(io)) == -22
    assert np.array_equal(rows, orig)
    # the device call checks its arguments before it touches a device
    assert L.cndp_gpu_cfwd(None, fib.h, ctypes.byref(b), 1, ctypes.byref(io), None) == -22
    # bin_of needs n_bins above in_lport and every known port, and at most CNDP_PART_BINS_MAX
    for in_lport, lports, n_bins, want in ((3, (), 3, -22), (3, (), 4, 0), (0, (9,), 9, -22), (0, (9,), 10, 0),
                                           (0, (255,), 4097, -22), (0, (255,), 256, 0)):
        rc, _ = cfwd_host(rows.reshape(-1).copy(), 1, R.FWD, in_lport=in_lport, lports=lports, n_bins=n_bins, stride=64, raw=True)
        assert rc == want, (in_lport, lports, n_bins, rc)
    # n == 0: nothing read, nothing written, in both modes; FWD needs no FIB
    for mode, f in ((R.FWD, None), (R.L3FWD, fib)):
        rc, r = cfwd_host(np.zeros(0, np.uint8), 0, mode, fib=f, lports=(0,), stride=64, raw=True)
        assert rc == 0 and not r["stats"].any() and len(r["tx_lport"]) == 0
    got = cfwd_host(rows.reshape(-1).copy(), 1, R.FWD, fib=None, lports=(0,), stride=64)
    assert got["tx_lport"].tolist() == [0]


def test_cfwd_under_sanitizers():
    """tests/cfwd_host/cfwd_san: cfwd.c (over fib.c / rib.c) built with
    -fsanitize=address,undefined in a program of its own, run as a child process:
    the helpers, both modes over heap slabs sized exactly to their last byte with
    every cut of the last frame, odd offsets, offsets past the end, random route
    changes with bursts between."""
    d = os.path.join(HERE, "cfwd_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "cfwd_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    flags = open(os.path.join(d, "Makefile")).read()
    assert "-fsanitize=address,undefined" in flags

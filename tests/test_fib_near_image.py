"""The near image of a DIR-24-8 FIB (cndp_amd/csrc/fib_near.c): its host builder
and the exported host walk (top -> /8 page -> /16 page -> tbl8, the LDS kernel's
rule) against the plain tbl24 / tbl8 lookup of the same FIB.  No device."""
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.fib import Fib

HERE = os.path.dirname(os.path.abspath(__file__))
DEF = 77
NESTED = [(0x14000000, 8, 1), (0x14100000, 12, 2), (0x14100000, 16, 3), (0x14108000, 17, 4),
          (0x1410C800, 24, 5), (0x1410C880, 25, 6), (0x1410C881, 32, 7)]
OTHER8 = [(0x1E010000, 16, 8), (0x28020300, 24, 9)]


@pytest.fixture(scope="module")
def sample():
    """2^20 random addresses, shared and left unchanged."""
    a = np.random.default_rng(2024).integers(0, 1 << 32, 1 << 20, dtype=np.uint32)
    a.setflags(write=False)
    return a


def mkfib():
    return Fib("near", N.CNE_FIB_DIR24_8, default_nh=DEF, max_routes=1024, nh_sz=N.CNE_FIB_DIR24_8_4B, num_tbl8=256)


def plain(fib, ips):
    t24, t8 = fib.image()
    e = t24[ips >> 8]
    x = (e & 1) == 1
    e = e.copy()
    e[x] = t8[(e[x] >> 1).astype(np.int64) * 256 + (ips[x] & 0xFF)]
    return (e >> 1).astype(np.uint64)


def edges(routes):
    out = []
    for ip, d, _ in routes:
        last = ip | ((1 << (32 - d)) - 1)
        out += [ip - 1, ip, ip + 1, last - 1, last, last + 1]
    return np.array([x & 0xFFFFFFFF for x in out], dtype=np.uint32)


def same(fib, sample, routes):
    """near == plain on the sample, the sample folded into the routed /8s, and every
    route's first and last address +-1."""
    ips = [sample, edges(routes)]
    for a in sorted({ip >> 24 for ip, _, _ in routes}):
        ips.append((sample[:1 << 16] & 0x00FFFFFF) | np.uint32(a << 24))
    ips = np.concatenate(ips)
    got, ref = fib.near_lookup(ips), plain(fib, ips)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, f"{len(bad)} differ, first {int(ips[bad[0]]):#x}: near {int(got[bad[0]])} plain {int(ref[bad[0]])}"
    return ref


def test_empty_fib(sample):
    fib = mkfib()
    ref = same(fib, sample, [])
    assert (ref == DEF).all()
    info = fib.near_info()
    assert info == dict(info, kib=1, fits=1, mid_used=0, pages_used=0, cap_kib=32)
    fib.close()


def test_nested_in_one_slash8(sample):
    fib = mkfib()
    for k, (ip, d, nh) in enumerate(NESTED):
        assert fib.add(ip, d, nh) == 0
        ref = same(fib, sample, NESTED[:k + 1])
    assert set(np.unique(ref)) == {DEF} | {nh for _, _, nh in NESTED}
    # one /8 page; 20.16/16 is the only /16 that is not uniform
    assert fib.near_info() == dict(fib.near_info(), kib=3, mid_used=1, pages_used=1, fits=1)
    fib.close()


def test_three_slash8s_deletes_and_reuse(sample):
    fib = mkfib()
    routes = NESTED + OTHER8
    for ip, d, nh in routes:
        assert fib.add(ip, d, nh) == 0
    same(fib, sample, routes)
    assert fib.near_info() == dict(fib.near_info(), kib=6, mid_used=3, mid_hwm=3, pages_used=2, page_hwm=2)
    # 40.2/16 uniform again: its page is freed, and 40/8's slot with it
    assert fib.delete(0x28020300, 24) == 0
    same(fib, sample, routes)
    assert fib.near_info() == dict(fib.near_info(), mid_used=2, pages_used=1, kib=6)
    # 30/8 uniform again: its slot is freed
    assert fib.delete(0x1E010000, 16) == 0
    same(fib, sample, routes)
    assert fib.near_info() == dict(fib.near_info(), mid_used=1, pages_used=1)
    # re-adds reuse the freed slots and page: the high-water marks stay
    for ip, d, nh in OTHER8:
        assert fib.add(ip, d, nh) == 0
    same(fib, sample, routes)
    assert fib.near_info() == dict(fib.near_info(), kib=6, mid_used=3, mid_hwm=3, pages_used=2, page_hwm=2, fits=1)
    fib.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_route_sets(sample, seed):
    rng = np.random.default_rng(seed)
    fib = mkfib()
    routes = []
    for _ in range(120):
        d = int(rng.integers(8, 33))
        ip = (int(rng.integers(0, 4)) * 0x11000000 + int(rng.integers(0, 1 << 22))) << 2
        ip &= (0xFFFFFFFF << (32 - d)) & 0xFFFFFFFF
        if (ip, d) not in {(a, b) for a, b, _ in routes} and fib.add(ip, d, len(routes) + 1) == 0:
            routes.append((ip, d, len(routes) + 1))
    same(fib, sample, routes)
    for ip, d, _ in routes[::3]:
        assert fib.delete(ip, d) == 0
    same(fib, sample, routes)
    fib.close()


def test_over_the_cap_is_reported(sample):
    """40 /24 routes in 40 /8s: 81 pages.  The walk stays exact; the image is reported
    as not fitting (the sanitizer program replays this for the bounds)."""
    fib = mkfib()
    routes = [(((50 + k) << 24) | (k << 16) | (k << 8), 24, 100 + k) for k in range(40)]
    for ip, d, nh in routes:
        assert fib.add(ip, d, nh) == 0
    same(fib, sample, routes)
    assert fib.near_info() == dict(fib.near_info(), kib=81, fits=0, mid_used=40, pages_used=40)
    fib.close()


def test_tables_without_a_directory():
    fib = Fib("wide", N.CNE_FIB_DIR24_8, default_nh=1, max_routes=16, nh_sz=N.CNE_FIB_DIR24_8_8B, num_tbl8=16)
    assert N.lib().cndp_fib_near_refresh(fib.h) == -95       # -ENOTSUP
    fib.close()


def test_near_image_under_sanitizers():
    """tests/fib_near_host/near_san: fib_near.c (over fib.c / rib.c) built with
    -fsanitize=address,undefined in a program of its own, run as a child process."""
    d = os.path.join(HERE, "fib_near_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "near_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    assert "-fsanitize=address,undefined" in open(os.path.join(d, "Makefile")).read()

"""The L4 chain past 1024 entries: cnet classify -> udp_input / tcp_input ->
cndp_gpu_bin_partition with one bin a PCB entry.  The 4096-entry tables of
test_l4_gpu.py and test_tcp_gpu.py (`full`, `distinct4096`, `one_port4096`,
`mixed4096`: same seeds, same frames, checked by those modules' own check()
against the restatements) and then the step they stop short of: every
socket's / connection's slice of `order` is its frames in arrival order, with
entries past index 1024 among them.  Also n_bins above the table's count."""
import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.l4 import PcbTable, port_net

import l4_ref as R
import tcp_ref as T
import test_l4_gpu as U
import test_tcp_gpu as TC
from helpers import cnet_fibs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(gpu):
    """(cl, local, other, udp): what test_tcp_gpu's check() takes; the first
    three are what test_l4_gpu's tests unpack."""
    from cndp_amd.classify import Classifier
    fib, fib6, routes, v6, v4vals, v6vals = cnet_fibs()
    cl = Classifier(0)
    cl.set_fib(fib, fib6)
    local = [ip for ip, d, _ in routes if d == 32]      # ip4_input's proto edge
    other = [routes[0][0] | 5, routes[1][0] | 9]        # forwarded, never taken
    udp = PcbTable(4)                                   # the UDP vector in front of tcp_input: empty
    udp.set_flags(punt_enabled=True, tcp_enabled=True)
    yield cl, local, other, udp
    udp.close()
    cl.close()


def assert_partition(cl, bin_of, nb):
    """cndp_gpu_bin_partition over `bin_of` (host uint16, every id < nb + 2):
    each bin's slice of `order` is its frames' indices in arrival order and
    bin_start ends at n.  Returns the ids that occur."""
    b = np.ascontiguousarray(bin_of, np.uint16)
    assert b.size == 0 or int(b.max()) < nb + 2
    start, order = cl.bin_partition(torch.from_numpy(b.view(np.int16)).to(f"cuda:{cl.device}"), nb)
    torch.cuda.synchronize()
    start, order = start.cpu().numpy().view(np.uint32), order.cpu().numpy().view(np.uint32)
    assert start[0] == 0 and start[nb + 2] == b.size
    for k in range(nb + 2):
        assert np.array_equal(order[start[k]:start[k + 1]], np.nonzero(b == k)[0]), k
    return np.unique(b)


@pytest.mark.parametrize("case", ["full", "distinct4096"])
def test_udp_4096_sockets_partition(env, gpu, case):
    """test_l4_gpu.test_table_shapes' 4096-entry tables: from the collision-heavy
    pool, and 4096 distinct ports of which every 64th is sent to."""
    cl, local, other, _ = env
    rng = np.random.default_rng(7)
    addrs, pp = U.pools(local)
    socks = U.sockets(local)
    if case == "full":
        tbl, ent = U.make_table(rng, 4096, local)
    else:
        k = 4096
        ports = rng.permutation(65535)[:k] + 1
        ent = np.zeros(k, R.ENTRY_DT)
        ent["lport"] = [port_net(int(p)) for p in ports]
        ent["laddr"] = rng.choice(addrs[:4] + [0], k)
        ent["flag"] = rng.choice([0, R.CHK], k)
        tbl = PcbTable(k)
        ent = R.fill_table(tbl, ent)
        socks = [(local[i % 4], int(p)) for i, p in enumerate(ports[:: k // 64])] + [(local[0], 0)]
    try:
        fr = pktgen.udp_socket_frames(257, socks, U.FOREIGN, seed=11, device=gpu, payload_lens=(0, 3, 18),
                                      cksum=("ok", "bad"), layout="packed", slot=128)
        got, want = U.check(cl, fr, tbl, ent)
        assert want["stats"][0] > 0
        nb = tbl.count()
        assert nb == 4096 > N.CNDP_BINS_MAX
        ids = assert_partition(cl, got["bin_of"], nb)
        assert np.array_equal(np.nonzero(got["l4edge"] == 0x11)[0], np.nonzero(got["bin_of"] < nb)[0])
        assert ((ids > 1024) & (ids < nb)).sum() >= 8 and nb + 1 in ids
    finally:
        tbl.close()


@pytest.mark.parametrize("case", ["one_port4096", "mixed4096"])
def test_tcp_4096_connections_partition(env, gpu, case):
    """test_tcp_gpu.test_table_shapes' 4096-entry tables: 4095 connections on
    one port plus its listener at index 2048 (every 42nd is sent to), and 4096
    mixed entries."""
    cl, local, other, _ = env
    rng = np.random.default_rng(17)
    prs = TC.pairs(local)
    if case == "mixed4096":
        tbl, ent = TC.make_table(rng, 4096, local)
    else:
        ent, prs = TC._one_port_table(local, 4096)
        tbl = PcbTable(4096)
        ent = R.fill_table(tbl, ent)
    try:
        fr = pktgen.tcp_socket_frames(257, prs, seed=21, device=gpu, payload_lens=(0, 3, 18), cksum=("ok", "ok", "bad"),
                                      layout="packed", slot=128)
        got, want, _ = TC.check(env, fr, tbl, ent)
        assert want["stats"][T.S_SEG] > 0 and want["stats"][T.S_CKSUM] > 0
        nb = tbl.count()
        assert nb == 4096 > N.CNDP_BINS_MAX
        ids = assert_partition(cl, got["bin_of"], nb)
        assert np.array_equal(np.nonzero(got["l4edge"] == T.E_SEG)[0], np.nonzero(got["bin_of"] < nb)[0])
        assert ((ids > 1024) & (ids < nb)).sum() >= 8 and nb in ids and nb + 1 in ids
        if case == "one_port4096":
            assert ((ids > 1024) & (ids < nb)).sum() > 30 and 2048 in ids
    finally:
        tbl.close()


@pytest.mark.parametrize("nb", [600, 1024])
def test_udp_n_bins_above_count(env, gpu, nb):
    """n_bins larger than the table's count: the extra bins move to nb and
    nb + 1, the sockets keep their indices, and the partition takes it."""
    cl, local, other, _ = env
    rng = np.random.default_rng(nb)
    tbl, ent = U.make_table(rng, 512, local)
    try:
        assert tbl.count() <= 512 < nb
        fr = pktgen.udp_socket_frames(1031, U.sockets(local, other), U.FOREIGN, seed=15, device=gpu,
                                      proto=(17, 17, 17, 6), cksum=("ok", "bad", "zero"), layout="packed", slot=128)
        got, want = U.check(cl, fr, tbl, ent, n_bins=nb)
        ids = assert_partition(cl, got["bin_of"], nb)
        assert nb in ids and nb + 1 in ids and (ids < 512).sum() >= 8 and not ((ids >= 512) & (ids < nb)).any()
    finally:
        tbl.close()


@pytest.mark.parametrize("nb", [600, 1024])
def test_tcp_n_bins_above_count(env, gpu, nb):
    """The same behind tcp_input."""
    cl, local, other, _ = env
    rng = np.random.default_rng(nb)
    tbl, ent = TC.make_table(rng, 512, local)
    try:
        assert tbl.count() <= 512 < nb
        fr = pktgen.tcp_socket_frames(1031, TC.pairs(local, other), seed=15, device=gpu,
                                      cksum=("ok", "ok", "bad", "zero"), data_off=TC.DOFFS, layout="packed", slot=128)
        got, want, _ = TC.check(env, fr, tbl, ent, n_bins=nb)
        ids = assert_partition(cl, got["bin_of"], nb)
        assert nb in ids and nb + 1 in ids and (ids < 512).sum() >= 8 and not ((ids >= 512) & (ids < nb)).any()
    finally:
        tbl.close()

"""Host side of the TCP connection demux (include/cndp_tcp.h, cndp_amd/csrc/pcb.c):
cndp_pcb_lookup_indexed (exact 4-tuple hash + per-port wildcard runs) against
the linear cndp_pcb_lookup and against the Python restatement of the
reference's rule, on tables built to reach every path of the index; its
generation tracking and return codes; the new exports; the checksum
restatement against the reference's recorded TCP verdicts
(tests/golden/tcp_cksum_ref.npz, tools/gen_tcp_cksum_golden.py); and the index
builder under the address / undefined-behaviour sanitizers in a stand-alone
program.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import PcbTable, addr_net, make_keys, port_net

import l4_ref as R
import tcp_ref as T

HERE = os.path.dirname(os.path.abspath(__file__))
ADDRS = [addr_net(a) for a in ("10.4.0.1", "10.4.0.2", "10.4.1.7", "198.18.0.1", "198.18.0.2")]
PORTS = [port_net(p) for p in (80, 443, 8080, 40000, 65535)]
NO_PORT = port_net(22)     # in no table: with listeners on every pool port, nothing else misses
OUTCOMES = {"exact", "wild1", "wild2", "miss"}


def _keys(rng, n, addrs=ADDRS, ports=PORTS):
    """Keys from the tables' own pool, with zero addresses and port 0 mixed in."""
    la = rng.choice(addrs + [0], n).astype(np.uint32)
    fa = rng.choice(addrs + [0], n).astype(np.uint32)
    lp = rng.choice(ports + [0, NO_PORT], n).astype(np.uint16)
    fp = rng.choice(ports + [0], n).astype(np.uint16)
    return make_keys(la, lp, fa, fp)


def _want(ent, keys):
    return np.array([R.lookup_ref(ent, int(k["laddr"]), int(k["faddr"]), int(k["lport"]), int(k["fport"]))
                     for k in keys], np.uint32)


def _outcomes(ent, keys):
    return {T.outcome(ent, int(k["laddr"]), int(k["faddr"]), int(k["lport"]), int(k["fport"])) for k in keys}


def _check(tbl, ent, keys):
    """indexed == linear == restatement; returns the answers."""
    got, lin, want = tbl.lookup_indexed(keys), tbl.lookup(keys), _want(ent, keys)
    bad = np.nonzero((got != want) | (lin != want))[0]
    assert len(bad) == 0, (f"{len(bad)} keys differ, first {keys[bad[0]]}: indexed {got[bad[0]]} "
                           f"linear {lin[bad[0]]} want {want[bad[0]]}")
    return got


@pytest.mark.parametrize("n", [0, 1, 513, 4096])
def test_indexed_lookup_parity_random_tables(n):
    """Seeded tables from a collision-heavy pool: few addresses and ports,
    duplicates, entries that differ only in fport, listeners, deleted entries."""
    rng = np.random.default_rng(7000 + n)
    tbl = PcbTable(max(n, 1))
    try:
        ent, dele = R.random_table(rng, n, ADDRS, PORTS, deleted_frac=0.1)
        if n >= 7:
            ent[0] = (0, 0, PORTS[0], 0, 0)                         # any/any listener
            ent[1] = (ADDRS[0], 0, PORTS[0], 0, 0)                  # bound listener
            ent[2] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[1], 0)    # connection
            ent[3] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[2], 0)    # differs only in fport
            ent[4] = ent[2]                                         # its duplicate: index 2 answers
            dele = np.union1d(dele[dele > 5], [5]).astype(np.int64)
        ent = R.fill_table(tbl, ent, dele)
        assert tbl.count() == n
        keys = _keys(rng, 600)
        if n >= 7:
            keys[0] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[1])      # exact, duplicated
            keys[1] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[2])      # the fport-only pair: entry 3
            keys[2] = (ADDRS[3], ADDRS[4], 0, 0)                    # port 0: a zeroed entry answers
        got = _check(tbl, ent, keys)
        if n >= 7:
            assert got[0] == 2 and got[1] == 3 and got[2] == 5
            # a table that never reaches one path of the index would hide a failure in it
            full = keys[(keys["laddr"] != 0) & (keys["faddr"] != 0)]
            assert _outcomes(ent, full) == OUTCOMES
            assert _outcomes(ent, keys[(keys["laddr"] == 0) | (keys["faddr"] == 0)]) >= {"exact", "wild1", "miss"}
    finally:
        tbl.close()


@pytest.mark.parametrize("n", [513, 4096])
def test_every_entry_on_one_port(n):
    """The TCP shape: one listening port, thousands of connections on it, its
    listeners somewhere in the middle of the vector."""
    rng = np.random.default_rng(7100 + n)
    port = PORTS[0]
    addrs = [addr_net(0xC6120000 + k) for k in range(1, 200)]
    ent = np.zeros(n, R.ENTRY_DT)
    ent["lport"] = port
    ent["laddr"] = ADDRS[0]
    ent["faddr"] = rng.choice(addrs, n)
    ent["fport"] = rng.integers(1, 65536, n)
    ent[n // 2] = (ADDRS[0], 0, port, 0, 0)          # bound listener
    ent[n // 2 + 7] = (0, 0, port, 0, 0)             # any/any listener, after it
    ent[n // 3] = ent[5]                             # duplicate of an earlier connection
    tbl = PcbTable(n)
    try:
        ent = R.fill_table(tbl, ent, [9])
        k = make_keys(ent["laddr"], ent["lport"], ent["faddr"], ent["fport"])   # every entry's own tuple
        extra = _keys(rng, 300, addrs=ADDRS + addrs[:3], ports=[port, PORTS[1]])
        keys = np.concatenate([k, extra])
        got = _check(tbl, ent, keys)
        assert got[n // 3] == 5 and got[5] == 5      # lowest index of equal tuples
        assert got[9] == 9                           # the zeroed entry's tuple is port 0 any/any: itself
        full = keys[(keys["laddr"] != 0) & (keys["faddr"] != 0)]
        assert _outcomes(ent, full) == OUTCOMES
    finally:
        tbl.close()


def _weak_hash_table():
    """4096 fully specified entries whose tuples differ only in what a weak
    hash drops: the address' high byte (256 values) and the foreign port's byte
    order (8 ports and their byte-swapped twins)."""
    ent = np.zeros(4096, R.ENTRY_DT)
    ports = [0x0102, 0x0304, 0x1234, 0x00FF, 0x7F80, 0x0150, 0xABCD, 0x0BB8]
    ports = ports + [((p & 0xFF) << 8) | (p >> 8) for p in ports]
    k = np.arange(4096)
    ent["laddr"] = 0x0004040A
    ent["faddr"] = 0x000012C6 | ((k & 0xFF).astype(np.uint32) << 24) | 0x00010000
    ent["lport"] = PORTS[0]
    ent["fport"] = np.array(ports, np.uint16)[k >> 8]
    return ent


def test_tuples_a_weak_hash_would_merge_and_generation_tracking():
    ent = _weak_hash_table()
    assert len(np.unique(ent[["laddr", "faddr", "lport", "fport"]])) == 4096
    rng = np.random.default_rng(7200)
    tbl = PcbTable(4096)
    try:
        half = 2048
        cur = R.fill_table(tbl, ent[:half])
        keys = make_keys(ent["laddr"], ent["lport"], ent["faddr"], ent["fport"])
        got = _check(tbl, cur, keys)
        assert (got[:half] == np.arange(half)).all() and (got[half:] == N.CNDP_PCB_NONE).all()
        # adds between lookups: the index follows the table's generation
        for e in ent[half:]:
            assert tbl.add_raw(int(e["laddr"]), int(e["faddr"]), int(e["lport"]), int(e["fport"]), 0) >= 0
        cur = ent.copy()
        got = _check(tbl, cur, keys)
        assert (got == np.arange(4096)).all()
        # deletes: the tuple stops answering, its neighbours in the hash keep theirs
        dele = rng.choice(4096, 300, replace=False)
        for i in dele:
            assert tbl.delete(int(i)) == 0
            cur[int(i)] = 0
        got = _check(tbl, cur, keys)
        assert (got[dele] == N.CNDP_PCB_NONE).all()
        keep = np.setdiff1d(np.arange(4096), dele)
        assert (got[keep] == keep).all()
        zero = make_keys([0x0004040A], [0], [0x010012C6], [7])
        assert _check(tbl, cur, zero)[0] == dele.min()       # deleted entries: any/any on port 0
        # keys with a zero address against fully specified entries: the whole-port walk
        part = keys[:64].copy()
        part["faddr"][:32] = 0
        part["laddr"][32:] = 0
        got = _check(tbl, cur, part)
        assert (got[:32] == keep[0]).all()                   # first live entry of the port, 1 wildcard
    finally:
        tbl.close()


def test_indexed_lookup_return_codes():
    L = N.lib()
    tbl = PcbTable(4)
    try:
        out = np.zeros(1, np.uint32)
        k = make_keys([1], [2], [3], [4])
        assert L.cndp_pcb_lookup_indexed(None, k.ctypes.data, 1, out.ctypes.data) == -22
        assert L.cndp_pcb_lookup_indexed(tbl.h, None, 1, out.ctypes.data) == -22
        assert L.cndp_pcb_lookup_indexed(tbl.h, k.ctypes.data, 1, None) == -22
        assert L.cndp_pcb_lookup_indexed(tbl.h, None, 0, None) == 0
        assert tbl.lookup_indexed(k)[0] == N.CNDP_PCB_NONE   # the empty table
        assert len(tbl.lookup_indexed(k[:0])) == 0
    finally:
        tbl.close()


def test_tcp_header_exports():
    """Every function include/cndp_tcp.h declares is exported by the built library."""
    names = N.l4_exported_symbols("cndp_tcp.h")
    assert set(names) == {"cndp_pcb_lookup_indexed", "cndp_gpu_tcp_input"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    # the call refuses what it cannot run, before it touches a device
    assert N.lib().cndp_gpu_tcp_input(None, None, None, None, None) == -22
    assert N.CNDP_L4_EDGE(N.CNDP_L4_NODE_TCP_INPUT, N.CNDP_TCP_INPUT_SEGMENT) == T.E_SEG
    assert ctypes.sizeof(N.TcpIo) == 64 and T.SEG_DT.itemsize == 16


def test_cksum_restatement_against_reference_tcp_golden():
    g = np.load(os.path.join(HERE, "golden", "tcp_cksum_ref.npz"))
    off, verify = g["off"], g["verify"]
    assert len(verify) >= 300 and set(np.unique(verify).tolist()) == {-1, 0}
    lens, kinds = set(), set()
    for i in range(len(verify)):
        s = g["data"][off[i]:off[i + 1]]
        lens.add(len(s) - int(g["l3_len"][i]))
        kinds.add(str(g["kind"][i]))
        ok = R.cksum_verify(R.View(s), 0, int(g["l3_len"][i]))
        assert ok == (verify[i] == 0), str(g["kind"][i])
    assert lens >= {20, 21, 35, 36, 37, 60, 83, 84, 85, 1460}
    assert kinds >= {"ok", "off_by_one", "zero_field_valid", "all_zero", "tot_lt_ihl", "claims_more"}
    zf = np.nonzero(g["kind"] == "zero_field_valid")[0]
    assert len(zf) and (verify[zf] == 0).all()   # TCP has no zero-field exemption to lean on: these sum right


def test_tcp_index_under_sanitizers():
    """tests/tcp_host/tcb_san: the TCP index builder and cndp_pcb_lookup_indexed
    built with -fsanitize=address,undefined in a program of its own, run as a
    child process."""
    d = os.path.join(HERE, "tcp_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "tcb_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    flags = open(os.path.join(d, "Makefile")).read()
    assert "-fsanitize=address,undefined" in flags

"""Host side of the UDP socket demux (include/cndp_l4.h, cndp_amd/csrc/pcb.c):
the PCB table's best-match lookup against a Python restatement of the
reference's rule (tests/l4_ref.py), its return codes, the new exports, the
checksum restatement against the reference's own recorded verdicts
(tests/golden/udp_cksum_ref.npz, tools/gen_udp_cksum_golden.py), and pcb.c
under the address / undefined-behaviour sanitizers in a stand-alone program.
No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cndp_amd import native as N
from cndp_amd.l4 import PcbTable, addr_net, make_keys, port_net

import l4_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ADDRS = [addr_net(a) for a in ("10.4.0.1", "10.4.0.2", "10.4.1.7", "198.18.0.1", "198.18.0.2")]
PORTS = [port_net(p) for p in (9, 53, 5000, 5001, 65535)]


def _keys(rng, n):
    """Keys from the same pool, with zero addresses and port 0 mixed in."""
    la = rng.choice(ADDRS + [0], n).astype(np.uint32)
    fa = rng.choice(ADDRS + [0], n).astype(np.uint32)
    lp = rng.choice(PORTS + [0], n).astype(np.uint16)
    fp = rng.choice(PORTS + [0], n).astype(np.uint16)
    return make_keys(la, lp, fa, fp)


@pytest.mark.parametrize("n", [0, 1, 7, 512, 4096])
def test_lookup_parity(n):
    rng = np.random.default_rng(100 + n)
    tbl = PcbTable(max(n, 1))
    try:
        ent, dele = R.random_table(rng, n, ADDRS, PORTS, deleted_frac=0.1)
        if n >= 7:   # the cases the pool must hold, whatever the draw
            ent[0] = (0, 0, PORTS[0], 0, 0)                         # any/any listener
            ent[1] = ent[0]                                         # its duplicate
            ent[2] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[1], 0)    # connected
            ent[3] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[2], 0)    # differs only in fport
            dele = np.union1d(dele[dele > 5], [5]).astype(np.int64)
        ent = R.fill_table(tbl, ent, dele)
        assert tbl.count() == n
        keys = _keys(rng, 400)
        if n >= 7:
            keys[0] = (ADDRS[0], ADDRS[1], PORTS[0], PORTS[2])      # the fport-only pair: entry 3
            keys[1] = (ADDRS[0], 0, PORTS[0], PORTS[2])             # zero faddr: fport ignored
            keys[2] = (ADDRS[3], ADDRS[4], 0, 0)                    # port 0: a zeroed entry answers
        got = tbl.lookup(keys)
        want = np.array([R.lookup_ref(ent, int(k["laddr"]), int(k["faddr"]), int(k["lport"]), int(k["fport"]))
                         for k in keys], np.uint32)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{len(bad)} keys differ, first {keys[bad[0]]}: got {got[bad[0]]} want {want[bad[0]]}"
        if n >= 7:
            assert got[0] == 3 and got[2] == 5
            assert (got != N.CNDP_PCB_NONE).sum() > 50
    finally:
        tbl.close()


def test_add_delete_return_codes():
    L = N.lib()
    h = ctypes.c_void_p()
    assert L.cndp_pcb_create(0, ctypes.byref(h)) == -22
    assert L.cndp_pcb_create(N.CNDP_PCB_MAX_ENTRIES + 1, ctypes.byref(h)) == -22
    tbl = PcbTable(3)
    try:
        assert [tbl.add(lport=5000 + i) for i in range(3)] == [0, 1, 2]
        assert tbl.add_raw(0, 0, 1, 0) == -28            # -ENOSPC: the vector is full
        assert tbl.delete(3) == -22                      # -EINVAL: outside the vector
        assert tbl.delete(1) == 0
        assert tbl.delete(1) == -2                       # -ENOENT: already deleted
        assert tbl.count() == 3                          # the zeroed entry stays
        assert tbl.add_raw(0, 0, 1, 0) == -28            # and its slot is not handed out again
        k = make_keys([ADDRS[0]], [port_net(5001)], [ADDRS[1]], [PORTS[0]])
        assert tbl.lookup(k)[0] == N.CNDP_PCB_NONE
        k["lport"] = 0
        assert tbl.lookup(k)[0] == 1                     # ... where it answers port 0
        assert L.cndp_pcb_add(None, None) == -22 and L.cndp_pcb_del(None, 0) == -22
        assert L.cndp_pcb_count(None) == -22 and L.cndp_pcb_set_flags(None, 1, 0) == -22
        tbl.set_flags(punt_enabled=False, tcp_enabled=True)
    finally:
        tbl.close()


def test_l4_header_exports():
    """Every function include/cndp_l4.h declares is exported by the built library."""
    names = N.l4_exported_symbols()
    assert set(names) >= {"cndp_pcb_create", "cndp_pcb_free", "cndp_pcb_add", "cndp_pcb_del", "cndp_pcb_set_flags",
                          "cndp_pcb_count", "cndp_pcb_lookup", "cndp_gpu_udp_input"}
    L = ctypes.CDLL(N.LIB_PATH)
    for nm in names:
        assert hasattr(L, nm), nm
    # the call refuses what it cannot run, before it touches a device
    assert N.lib().cndp_gpu_udp_input(None, None, None, None, None) == -22


def test_cksum_restatement_against_reference_golden():
    g = np.load(os.path.join(HERE, "golden", "udp_cksum_ref.npz"))
    off, verify = g["off"], g["verify"]
    assert len(verify) >= 300 and set(np.unique(verify).tolist()) == {-1, 0}
    lens = set()
    for i in range(len(verify)):
        s = g["data"][off[i]:off[i + 1]]
        lens.add(len(s) - int(g["l3_len"][i]))
        ok = R.cksum_verify(R.View(s), 0, int(g["l3_len"][i]))
        assert ok == (verify[i] == 0), str(g["kind"][i])
    assert lens >= {8, 9, 15, 16, 17, 63, 64, 65, 1472}


def test_pcb_under_sanitizers():
    """tests/l4_host/pcb_san: pcb.c built with -fsanitize=address,undefined in a
    program of its own, run as a child process."""
    d = os.path.join(HERE, "l4_host")
    subprocess.run(["make", "-s", "-C", d], check=True, timeout=300)
    r = subprocess.run([os.path.join(d, "pcb_san")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    flags = open(os.path.join(d, "Makefile")).read()
    assert "-fsanitize=address,undefined" in flags


def test_derived_selection_types_match_reference_p_nxt():
    """The packet types the derived selection takes are the ptype node's own
    p_nxt entries for ip4_input (tests/golden/ptype_ref.json), in the
    restatement and in the kernel source alike."""
    from helpers import ptype_ref
    ref = ptype_ref()
    want = sorted(int(k, 16) for k, v in ref["pnxt"].items() if v == ref["ptype_next"]["PTYPE_NEXT_IP4_INPUT"])
    assert sorted(R.IP4_INPUT_TYPES) == want
    src = open(os.path.join(HERE, "..", "cndp_amd", "csrc", "cndp_l4.hip")).read()
    body = src[src.index("ptype_is_ip4_input"):]
    body = body[:body.index("}")]
    import re
    assert sorted(int(x, 16) for x in re.findall(r"(0x0[0-9a-f]{3})u", body)) == want

"""cndpfwd's fwd and l3fwd modes (include/cndp_cfwd.h): the l3fwd FIB, the next
hop packing, and the arrays of Classifier.cndpfwd.

    fib = l3fwd_fib()                                   # l3fwd_fib_init's DUMMY FIB
    route_add(fib, 0xC6120000, 24, "02:00:00:00:00:01", 1)
    r = c.cndpfwd(frames, N.CNDP_CFWD_L3FWD, fib=fib, in_lport=0, lports=(0, 1))
    r["tx_lport"], r["nh"], r["echoed"], r["bin_of"], r["stats"]
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as N
from .acl import default_n_bins, lport_mask
from .fib import Fib


class L3fwdFib(Fib):
    """cndp_cfwd_fib_create: a CNE_FIB_DUMMY FIB with max_routes 1 << 16 and
    the default next hop 0xFFFFFFFFFFFF (l3-fwd.c:96-103)."""

    def __init__(self, name="l3fwd_fib"):  # noqa: the C helper makes the FIB
        self._L = N.lib()
        self.h = self._L.cndp_cfwd_fib_create(name.encode() if name is not None else None)
        if not self.h:
            raise ValueError("cndp_cfwd_fib_create failed")
        self.type = N.CNE_FIB_DUMMY
        self.default_nh = N.CNDP_CFWD_DEFAULT_NH


def l3fwd_fib(name: str = "l3fwd_fib") -> Fib:
    return L3fwdFib(name)


def mac_bytes(mac) -> bytes:
    """Six octets from "aa:bb:cc:dd:ee:ff", bytes or a sequence of six ints."""
    b = bytes(int(x, 16) for x in mac.split(":")) if isinstance(mac, str) else bytes(mac)
    if len(b) != 6:
        raise ValueError(f"a MAC has six octets, not {len(b)}")
    return b


def nexthop(mac, port: int) -> int:
    """cndp_cfwd_nexthop: (port << 48) | inet_mtoh64(mac)  (l3-fwd.c:64-67)."""
    return N.lib().cndp_cfwd_nexthop(mac_bytes(mac), port & 0xFFFF)


def route_add_raw(fib: Fib, ip: int, depth: int, mac, port: int) -> int:
    """cndp_cfwd_route_add; returns its result (0 or -errno).  A port above
    0xFFFF is refused here as the C call refuses one above 0x7FFF."""
    if not 0 <= port <= 0xFFFF:
        return -22
    return N.lib().cndp_cfwd_route_add(fib.h, ip & 0xFFFFFFFF, depth, mac_bytes(mac), port)


def route_add(fib: Fib, ip: int, depth: int, mac, port: int) -> None:
    N.check(route_add_raw(fib, ip, depth, mac, port), "cndp_cfwd_route_add")


def cfwd_io(io_arrays: dict, ptr, in_lport: int, lports, n_bins: int, sel=None) -> "N.CfwdIo":
    """struct cndp_cfwd_io over `io_arrays` (nh, tx_lport, echoed, bin_of,
    stats); ptr maps an array to its address (or None)."""
    io = N.CfwdIo()
    io.sel = ptr(sel)
    io.in_lport = in_lport
    for k, w in enumerate(lport_mask(lports)):
        io.lport_mask[k] = w
    io.nh, io.tx_lport = ptr(io_arrays.get("nh")), ptr(io_arrays.get("tx_lport"))
    io.echoed, io.bin_of = ptr(io_arrays.get("echoed")), ptr(io_arrays.get("bin_of"))
    io.n_bins, io.stats = n_bins, ptr(io_arrays.get("stats"))
    return io


def alloc_cfwd_outputs(n: int, device) -> dict:
    """The output arrays of cndp_gpu_cfwd as torch tensors."""
    import torch
    m = max(n, 1)
    return {"nh": torch.empty(m, dtype=torch.int64, device=device)[:n],
            "tx_lport": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "echoed": torch.empty(m, dtype=torch.uint8, device=device)[:n],
            "bin_of": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "stats": torch.zeros(N.CNDP_CFWD_NSTATS, dtype=torch.int64, device=device)}


def cfwd_host(slab: np.ndarray, n: int, mode: int, fib: Fib | None = None, in_lport: int = 0, lports=(),
              n_bins: int | None = None, sel=None, stride: int = 0, offsets=None, data_off: int = 0, stats=None,
              slab_len: int | None = None, raw: bool = False):
    """cndp_cfwd_host over host arrays: the stage's rule on the calling thread;
    `slab` (a contiguous uint8 array) is edited in place.  Returns nh (uint64),
    tx_lport (uint16), echoed (uint8), bin_of (uint16) and stats
    (uint64[CNDP_CFWD_NSTATS], accumulated into `stats` when given); with
    raw=True the call's result code and the same dict, error or not."""
    assert slab.dtype == np.uint8 and slab.flags["C_CONTIGUOUS"]
    m = max(n, 1)
    out = {"nh": np.zeros(m, np.uint64), "tx_lport": np.zeros(m, np.uint16), "echoed": np.zeros(m, np.uint8),
           "bin_of": np.zeros(m, np.uint16),
           "stats": np.zeros(N.CNDP_CFWD_NSTATS, np.uint64) if stats is None else np.array(stats, np.uint64)}

    def ptr(a):
        return None if a is None else a.ctypes.data

    sel = None if sel is None else np.ascontiguousarray(sel, np.uint8)
    offsets = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
    b = N.Batch()
    b.n, b.slab, b.slab_len = n, slab.ctypes.data, slab.size if slab_len is None else slab_len
    b.stride, b.data_off, b.offsets = stride, data_off, ptr(offsets)
    if n_bins is None:
        n_bins = default_n_bins(in_lport, lports)
    io = cfwd_io(out, ptr, in_lport, lports, n_bins, sel=sel)
    rc = N.lib().cndp_cfwd_host(fib.h if fib is not None else None, ctypes.byref(b), mode, ctypes.byref(io))
    res = {k: (v if k == "stats" else v[:n]) for k, v in out.items()}
    res["n_bins"] = n_bins
    if raw:
        return rc, res
    N.check(rc, "cndp_cfwd_host")
    return res

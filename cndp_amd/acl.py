"""cndpfwd's ACL forwarding mode (include/cndp_acl.h): the rule table and the
output arrays of Classifier.acl_fwd.

    acl = AclTable()
    acl.add_init_rules()                    # or acl.add(src, 24, dst, 32, deny=True) ...
    acl.build()                             # rules take effect here
    r = c.acl_fwd(frames, acl, mode=N.CNDP_ACL_STRICT, swap=True, lports=(0, 1))
    r["verdict"], r["result"], r["tx_lport"], r["bin_of"], r["stats"]
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native as N


def lport_mask(lports) -> list:
    """The 256-bit map of struct cndp_acl_io from an iterable of port numbers."""
    m = [0, 0, 0, 0]
    for p in lports:
        if not 0 <= int(p) < 256:
            raise ValueError(f"lport {p} is not in 0..255")
        m[int(p) >> 6] |= 1 << (int(p) & 63)
    return m


def acl_io(io_arrays: dict, ptr, in_lport: int, lports, n_bins: int, sel=None, length=None) -> "N.AclIo":
    """struct cndp_acl_io over `io_arrays` (result, verdict, tx_lport, bin_of,
    stats); ptr maps an array to its address (or None)."""
    io = N.AclIo()
    io.sel, io.len = ptr(sel), ptr(length)
    io.in_lport = in_lport
    for k, w in enumerate(lport_mask(lports)):
        io.lport_mask[k] = w
    io.result, io.verdict = ptr(io_arrays.get("result")), ptr(io_arrays.get("verdict"))
    io.tx_lport, io.bin_of = ptr(io_arrays.get("tx_lport")), ptr(io_arrays.get("bin_of"))
    io.n_bins, io.stats = n_bins, ptr(io_arrays.get("stats"))
    return io


def default_n_bins(in_lport: int, lports) -> int:
    return max([in_lport, *[int(p) for p in lports]]) + 1


class AclTable:
    """cndp_acl_* (include/cndp_acl.h): acl-func.c's rule vector and the image
    lookups read.  Rules added or cleared take effect at the next build()."""

    def __init__(self):
        self._L = N.lib()
        h = ctypes.c_void_p()
        N.check(self._L.cndp_acl_tbl_create(ctypes.byref(h)), "cndp_acl_tbl_create")
        self.h = h

    def close(self):
        if self.h:
            self._L.cndp_acl_tbl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_raw(self, src_addr: int, src_msk: int, dst_addr: int, dst_msk: int, deny: bool = False) -> int:
        """cndp_acl_add; returns its result (0 or -errno)."""
        r = N.AclRule(src_addr & 0xFFFFFFFF, dst_addr & 0xFFFFFFFF, src_msk & 0xFF, dst_msk & 0xFF, 1 if deny else 0, 0)
        return self._L.cndp_acl_add(self.h, ctypes.byref(r))

    def add(self, src_addr: int, src_msk: int, dst_addr: int, dst_msk: int, deny: bool = False) -> None:
        N.check(self.add_raw(src_addr, src_msk, dst_addr, dst_msk, deny), "cndp_acl_add")

    def add_many(self, src_addr, src_msk, dst_addr, dst_msk, deny) -> None:
        for s, sm, d, dm, dn in zip(np.asarray(src_addr).tolist(), np.asarray(src_msk).tolist(),
                                    np.asarray(dst_addr).tolist(), np.asarray(dst_msk).tolist(),
                                    np.asarray(deny).tolist()):
            self.add(s, sm, d, dm, bool(dn))

    def add_init_rules(self) -> None:
        N.check(self._L.cndp_acl_add_init_rules(self.h), "cndp_acl_add_init_rules")

    def clear(self) -> None:
        N.check(self._L.cndp_acl_clear(self.h), "cndp_acl_clear")

    def count(self) -> int:
        return N.check(self._L.cndp_acl_count(self.h), "cndp_acl_count")

    def get(self, idx: int):
        """Rule idx as (src_addr, src_msk, dst_addr, dst_msk, deny), or None past the end."""
        r = N.AclRule()
        if self._L.cndp_acl_get(self.h, idx, ctypes.byref(r)) < 0:
            return None
        return (r.src_addr, r.src_msk, r.dst_addr, r.dst_msk, bool(r.deny))

    def build_raw(self) -> int:
        """cndp_acl_build; returns its result (0 or -errno)."""
        return self._L.cndp_acl_build(self.h)

    def build(self) -> None:
        N.check(self.build_raw(), "cndp_acl_build")

    def classify_host(self, slab: np.ndarray, n: int, mode: int = N.CNDP_ACL_STRICT, swap: bool = False,
                      in_lport: int = 0, lports=(), n_bins: int | None = None, sel=None, length=None,
                      stride: int = 0, offsets=None, data_off: int = 0, stats=None, slab_len: int | None = None,
                      raw: bool = False):
        """cndp_acl_classify_host over host arrays: the stage's rule on the calling
        thread; `slab` (a contiguous uint8 array) is written in place with swap.
        Returns result (uint32), verdict, tx_lport (uint8), bin_of (uint16) and
        stats (uint64[CNDP_ACL_NSTATS], accumulated into `stats` when given); with
        raw=True the call's result code and the same dict, error or not."""
        assert slab.dtype == np.uint8 and slab.flags["C_CONTIGUOUS"]
        m = max(n, 1)
        out = {"result": np.zeros(m, np.uint32), "verdict": np.zeros(m, np.uint8), "tx_lport": np.zeros(m, np.uint8),
               "bin_of": np.zeros(m, np.uint16),
               "stats": np.zeros(N.CNDP_ACL_NSTATS, np.uint64) if stats is None else np.array(stats, np.uint64)}
        keep = []

        def ptr(a):
            return None if a is None else a.ctypes.data

        if sel is not None:
            keep.append(np.ascontiguousarray(sel, np.uint8))
        if length is not None:
            keep.append(np.ascontiguousarray(length, np.uint16))
        b = N.Batch()
        b.n, b.slab, b.slab_len = n, slab.ctypes.data, slab.size if slab_len is None else slab_len
        b.stride, b.data_off = stride, data_off
        if offsets is not None:
            keep.append(np.ascontiguousarray(offsets, np.uint64))
            b.offsets = keep[-1].ctypes.data
        if n_bins is None:
            n_bins = default_n_bins(in_lport, lports)
        io = acl_io(out, ptr, in_lport, lports, n_bins,
                    sel=keep[0] if sel is not None else None,
                    length=keep[1 if sel is not None else 0] if length is not None else None)
        rc = self._L.cndp_acl_classify_host(self.h, ctypes.byref(b), mode, N.CNDP_ACL_F_MAC_SWAP if swap else 0,
                                            ctypes.byref(io))
        res = {k: (v if k == "stats" else v[:n]) for k, v in out.items()}
        res["n_bins"] = n_bins
        if raw:
            return rc, res
        N.check(rc, "cndp_acl_classify_host")
        return res


def alloc_acl_outputs(n: int, device) -> dict:
    """The output arrays of cndp_gpu_acl_fwd as torch tensors."""
    import torch
    m = max(n, 1)
    return {"result": torch.empty(m, dtype=torch.int32, device=device)[:n],
            "verdict": torch.empty(m, dtype=torch.uint8, device=device)[:n],
            "tx_lport": torch.empty(m, dtype=torch.uint8, device=device)[:n],
            "bin_of": torch.empty(m, dtype=torch.int16, device=device)[:n],
            "stats": torch.zeros(N.CNDP_ACL_NSTATS, dtype=torch.int64, device=device)}

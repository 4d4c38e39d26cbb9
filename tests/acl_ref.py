"""A vectorised restatement of cndpfwd's ACL mode (CNDP v25.08.0,
examples/cndpfwd/acl-func.c), written from the reference's text and pinned to
its compiled ACL library by tests/golden/acl_ref.npz:

  classify()      cne_acl_classify's result under acl_tbl_write_rule's
                  priorities: the userdata of the lowest-index rule whose two
                  prefixes cover the packet, or 0 -- a first-match brute force
  acl_fwd_ref()   acl_fwd_test per frame: validate_ipv4_pkt (:244-282), the
                  classify at mtod + 23, the forward decision (:358-384), the
                  destination port, MAC_SWAP and the three counters

and the helpers the tests share: the golden sets, a frame builder, slab layouts.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DENY = 0xF0000000
NONE, PREFILTER, DENIED, FORWARD = 0, 1, 2, 3
STRICT, PERMISSIVE = 0, 1
LPORT_NONE = 0xFF
_golden = None


def golden(name: str) -> dict:
    """Rule set `name` ('a', 'b', 'b0') of acl_ref.npz: rules, packets, recorded results."""
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(HERE, "golden", "acl_ref.npz")))
    g = _golden
    return {"rules": {k: g[f"{name}_{k}"] for k in ("src_addr", "src_msk", "dst_addr", "dst_msk", "deny")},
            "psrc": g[f"{name}_psrc"], "pdst": g[f"{name}_pdst"], "res": g[f"{name}_res"]}


def rules_of(rows) -> dict:
    """Rule arrays from (src_addr, src_msk, dst_addr, dst_msk, deny) rows."""
    r = np.array(rows, np.uint64).reshape(-1, 5)
    return {"src_addr": r[:, 0].astype(np.uint32), "src_msk": r[:, 1].astype(np.uint8),
            "dst_addr": r[:, 2].astype(np.uint32), "dst_msk": r[:, 3].astype(np.uint8), "deny": r[:, 4].astype(np.uint8)}


def cat_rules(*rs) -> dict:
    return {k: np.concatenate([r[k] for r in rs]) for k in rs[0]}


def masks(lens) -> np.ndarray:
    lens = np.asarray(lens, np.uint64)
    return ((np.uint64(0xFFFFFFFF) << (np.uint64(32) - lens)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def match_matrix(rules: dict, src, dst) -> np.ndarray:
    """[packet, rule] -> does the rule cover the packet."""
    src, dst = np.asarray(src, np.uint32)[:, None], np.asarray(dst, np.uint32)[:, None]
    ms, md = masks(rules["src_msk"])[None, :], masks(rules["dst_msk"])[None, :]
    return (((src ^ rules["src_addr"][None, :]) & ms) == 0) & (((dst ^ rules["dst_addr"][None, :]) & md) == 0)


def first_match(rules: dict, src, dst) -> np.ndarray:
    """Index of the first rule covering each packet, -1 for none."""
    src, dst = np.asarray(src, np.uint32), np.asarray(dst, np.uint32)
    nr = len(rules["src_addr"])
    out = np.full(len(src), -1, np.int64)
    if nr == 0:
        return out
    step = max(1, (1 << 22) // nr)
    for lo in range(0, len(src), step):
        m = match_matrix(rules, src[lo:lo + step], dst[lo:lo + step])
        k = m.argmax(1)
        out[lo:lo + step] = np.where(m[np.arange(len(k)), k], k, -1)
    return out


def classify(rules: dict, src, dst) -> np.ndarray:
    k = first_match(rules, src, dst)
    deny = rules["deny"].astype(bool)[np.maximum(k, 0)]
    return np.where(k < 0, 0, k + np.where(deny, DENY, 1)).astype(np.uint32)


def frames(src, dst, dmac5=None, ver_ihl=0x45, tot=46, etype=0x0800, size=64, seed=1) -> np.ndarray:
    """(n, size) frames: random bytes with the fields the stage reads set --
    destination MAC byte 5, the ethertype, version/IHL, total_length and the
    addresses at frame bytes 26 and 30 (whatever the IHL)."""
    src, dst = np.asarray(src, np.uint32), np.asarray(dst, np.uint32)
    n = len(src)
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, size), dtype=np.uint8)
    if dmac5 is not None:
        f[:, 5] = dmac5
    f[:, 12], f[:, 13] = etype >> 8, etype & 0xFF
    f[:, 14] = ver_ihl
    tot = np.broadcast_to(np.asarray(tot, np.uint16), (n,))
    f[:, 16], f[:, 17] = tot >> 8, tot & 0xFF
    for k in range(4):
        f[:, 26 + k] = (src >> (24 - 8 * k)) & 0xFF
        f[:, 30 + k] = (dst >> (24 - 8 * k)) & 0xFF
    return f


def layout(rows, kind: str, seed: int = 3):
    """Place the frames `rows` in a slab: 'packed' (their own size as the
    stride), 'stride68', 'umem' (2 KiB slots, data_off 256) or 'offsets' (an offsets array,
    frames cut to mixed sizes of at least 34 bytes at byte-granular places).
    Returns (slab, dict(stride=, offsets=, data_off=))."""
    n, size = rows.shape
    rng = np.random.default_rng(seed)
    if kind == "packed":
        return rows.reshape(-1).copy(), dict(stride=size, offsets=None, data_off=0)
    if kind == "stride68":                               # 4-byte but not 16-byte aligned frames
        slab = rng.integers(0, 256, (n, 68), dtype=np.uint8)
        slab[:, :size] = rows
        return slab.reshape(-1), dict(stride=68, offsets=None, data_off=0)
    if kind == "umem":
        slab = rng.integers(0, 256, (n, 2048), dtype=np.uint8)
        slab[:, 256:256 + size] = rows
        return slab.reshape(-1), dict(stride=2048, offsets=None, data_off=256)
    assert kind == "offsets"
    sizes = rng.choice([34, 35, 60, 61, 64], n)
    gaps = rng.choice([0, 1, 2, 3, 4, 16], n)
    offs = np.cumsum(sizes + gaps) - sizes + 16          # data_off 3 below: still inside the slab
    slab = rng.integers(0, 256, int(offs[-1] + sizes[-1]) + 8 if n else 8, dtype=np.uint8)
    for i in range(n):
        slab[offs[i]:offs[i] + sizes[i]] = rows[i, :sizes[i]]
    return slab, dict(stride=0, offsets=(offs - 3).astype(np.uint64), data_off=3)


def acl_fwd_ref(slab, n, rules: dict, mode=STRICT, swap=False, in_lport=0, lports=(), n_bins=None, sel=None,
                length=None, stride=0, offsets=None, data_off=0, stats=None, slab_len=None) -> dict:
    """acl_fwd_test over n frames.  Returns result, verdict, tx_lport, bin_of,
    stats (accumulated onto `stats`) and `slab`, the slab as the stage leaves it.
    Bytes at or past slab_len read as zero."""
    slab = np.ascontiguousarray(slab, np.uint8)
    slab_len = len(slab) if slab_len is None else slab_len
    at = (np.asarray(offsets, np.uint64) if offsets is not None else np.arange(n, dtype=np.uint64) * np.uint64(stride))
    at = at.astype(np.int64) + data_off
    padded = np.concatenate([slab[:slab_len], np.zeros(64, np.uint8)])

    def byte(k):
        x = at + k
        return padded[np.minimum(x, slab_len)].astype(np.uint32)    # index slab_len is a zero

    be32 = lambda k: byte(k) << 24 | byte(k + 1) << 16 | byte(k + 2) << 8 | byte(k + 3)  # noqa: E731
    taken = np.ones(n, bool) if sel is None else np.asarray(sel)[:n] != 0
    link = np.ones(n, bool) if length is None else np.asarray(length)[:n].astype(np.int64) >= 20
    vi, tot = byte(14), byte(16) << 8 | byte(17)
    valid = link & ((vi >> 4) == 4) & ((vi & 15) >= 5) & (tot >= 20)
    cls = taken & valid
    res = np.where(cls, classify(rules, be32(26), be32(30)), 0).astype(np.uint32)
    deny, permit = (res & DENY) != 0, res != 0
    fwd = cls & ~deny & (permit | (mode == PERMISSIVE))
    verdict = np.where(~taken, NONE, np.where(~cls, PREFILTER, np.where(fwd, FORWARD, DENIED))).astype(np.uint8)
    dmac5 = byte(5)
    known = np.zeros(256, bool)
    known[list(lports)] = True
    tx = np.where(fwd, np.where(known[dmac5], dmac5, in_lport), LPORT_NONE).astype(np.uint8)
    if n_bins is None:
        n_bins = max([in_lport, *lports]) + 1
    bin_of = np.where(fwd, tx, np.where(verdict == DENIED, n_bins, n_bins + 1)).astype(np.uint16)
    st = np.zeros(3, np.uint64) if stats is None else np.array(stats, np.uint64)
    st += np.array([np.count_nonzero(verdict == v) for v in (PREFILTER, DENIED, FORWARD)], np.uint64)
    after = slab.copy()
    if swap:
        for i in np.nonzero(fwd)[0]:
            a = at[i]
            after[a:a + 6], after[a + 6:a + 12] = slab[a + 6:a + 12], slab[a:a + 6]
    return {"result": res, "verdict": verdict, "tx_lport": tx, "bin_of": bin_of, "stats": st, "slab": after,
            "n_bins": n_bins}


def big_rules(seed: int = 7):
    """100000 rules: 90000 distinct /32:/32 allow / deny pairs, then 10000 of
    mixed lengths over the same addresses.  Returns (rules, psrc, pdst): 512
    packets drawn from the rules (bits beyond the prefix randomised) and 64 of
    them turned into misses."""
    rng = np.random.default_rng(seed)
    k = np.arange(90000, dtype=np.uint32)
    a = {"src_addr": np.uint32(0x0B000000) + k * np.uint32(7), "src_msk": np.full(90000, 32, np.uint8),
         "dst_addr": np.uint32(0xC0A80000) + k * np.uint32(13), "dst_msk": np.full(90000, 32, np.uint8),
         "deny": (k % 3 == 0).astype(np.uint8)}
    j = rng.integers(0, 90000, 10000)
    lens = np.array([8, 16, 24, 31, 32, 0], np.uint8)
    sm, dm = rng.choice(lens[:5], 10000), rng.choice(lens, 10000)
    b = {"src_addr": a["src_addr"][j] ^ np.uint32(0x55), "src_msk": sm, "dst_addr": a["dst_addr"][j] ^ np.uint32(0xAA),
         "dst_msk": dm, "deny": rng.integers(0, 2, 10000).astype(np.uint8)}
    rules = cat_rules(a, b)
    pick = np.concatenate([rng.integers(0, 90000, 256), rng.integers(90000, 100000, 256)])
    ms, md = masks(rules["src_msk"][pick]), masks(rules["dst_msk"][pick])
    rs = rng.integers(0, 1 << 32, 512, dtype=np.uint64).astype(np.uint32)
    rd = rng.integers(0, 1 << 32, 512, dtype=np.uint64).astype(np.uint32)
    psrc = (rules["src_addr"][pick] & ms) | (rs & ~ms)
    pdst = (rules["dst_addr"][pick] & md) | (rd & ~md)
    psrc[::8] ^= np.uint32(0x80000000)
    return rules, psrc, pdst

"""cndpfwd's ACL mode on the GPU (cndp_gpu_acl_fwd, include/cndp_acl.h):
result, verdict, tx_lport, bin_of, the counters and the WHOLE slab must equal
the Python restatement (tests/acl_ref.py, pinned to the compiled reference by
tests/golden/acl_ref.npz) for every frame.  Shapes are the smallest that can
still go wrong: no frame, one frame, a wave and its neighbours, more than one
256-lane block; packed 64-byte slots (16-byte aligned frames), 68-byte slots
(4-byte aligned), the UMEM stride, byte-granular offsets; frames that straddle
and lie past the end of the slab; a table at the rule cap.

Rule set (b) of the issue is two sets here, b (no /0:/0 rule, a tenth of the
packets match nothing) and b0 (the /0:/0 rule at index 150): see
test_acl_host.py."""
import numpy as np
import pytest
import torch

from cndp_amd import native as N
from cndp_amd import pktgen
from cndp_amd.acl import AclTable, alloc_acl_outputs

import acl_ref as A

pytestmark = pytest.mark.gpu
SETS = ("a", "b", "b0")
KEYS = ("result", "verdict", "tx_lport", "bin_of", "stats")
DT = {"result": np.uint32, "verdict": np.uint8, "tx_lport": np.uint8, "bin_of": np.uint16, "stats": np.uint64}


def table(rules: dict) -> AclTable:
    t = AclTable()
    t.add_many(rules["src_addr"], rules["src_msk"], rules["dst_addr"], rules["dst_msk"], rules["deny"])
    t.build()
    return t


@pytest.fixture(scope="module")
def cl(gpu):
    from cndp_amd.classify import Classifier
    c = Classifier(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tables(gpu):
    ts = {s: table(A.golden(s)["rules"]) for s in SETS}
    yield ts
    for t in ts.values():
        t.close()


def to_frames(slab, n, lay, dev="cuda:0"):
    offs = None if lay["offsets"] is None else torch.from_numpy(lay["offsets"].astype(np.int64)).to(dev)
    return pktgen.Frames(torch.from_numpy(slab.copy()).to(dev), n, stride=lay["stride"], offsets=offs,
                         data_off=lay["data_off"])


def run(cl, t, rules, slab, n, lay, acl=None, stats0=None, **kw):
    """One acl_fwd call against the restatement on the same bytes: outputs, the
    counters and the whole slab.  Returns (got, want, the result tensors)."""
    fr = to_frames(slab, n, lay)
    dev_kw = dict(kw)
    for k, dt in (("sel", np.uint8), ("length", np.int16)):
        if kw.get(k) is not None:
            dev_kw[k] = torch.from_numpy(np.ascontiguousarray(kw[k]).astype(dt)).to(fr.slab.device)
    res = cl.acl_fwd(fr, t, acl=acl, **dev_kw)
    torch.cuda.synchronize()
    got = {k: res[k].cpu().numpy().view(DT[k]).copy() for k in KEYS}
    want = A.acl_fwd_ref(slab, n, rules, stats=stats0, **kw, **lay)
    for k in KEYS:
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, f"{k}: {len(bad)} differ, first at {bad[0]}: got {got[k][bad[0]]} want {want[k][bad[0]]}"
    after = fr.slab.cpu().numpy()
    bad = np.nonzero(after != want["slab"])[0]
    assert len(bad) == 0, f"slab: {len(bad)} bytes differ, first at {bad[0]}"
    return got, want, res


@pytest.mark.parametrize("swap", (False, True))
@pytest.mark.parametrize("mode", (A.STRICT, A.PERMISSIVE))
@pytest.mark.parametrize("name", SETS)
def test_golden_rule_sets(cl, tables, name, mode, swap):
    g = A.golden(name)
    rows = A.frames(g["psrc"], g["pdst"], dmac5=np.arange(2048) % 6)
    got, want, _ = run(cl, tables[name], g["rules"], rows.reshape(-1), 2048, dict(stride=64, offsets=None, data_off=0),
                       mode=mode, swap=swap, in_lport=5, lports=(0, 1, 2, 3))
    assert np.array_equal(got["result"], g["res"]), "differs from the results the reference recorded"
    assert set(np.unique(want["verdict"])) == {A.DENIED, A.FORWARD}


@pytest.mark.parametrize("with_sel", (False, True))
@pytest.mark.parametrize("kind", ("packed", "stride68", "umem", "offsets"))
def test_wave_block_and_slab_edges(cl, tables, kind, with_sel):
    g = A.golden("a")
    seen = set()
    for n in (0, 1, 63, 64, 65, 257, 1000):
        rows = A.frames(g["psrc"][:n], g["pdst"][:n], dmac5=np.arange(n) % 5, seed=n + 1)
        rows[3::11, 14] = 0x35                                      # a few that validate_ipv4_pkt drops
        slab, lay = A.layout(rows, kind, seed=n)
        sel = (np.arange(n) % 4 != 2).astype(np.uint8) if with_sel else None
        kw = dict(mode=A.STRICT, swap=True, in_lport=4, lports=(0, 1, 2), sel=sel)
        _, want, _ = run(cl, tables["a"], g["rules"], slab, n, lay, **kw)
        seen |= set(want["verdict"].tolist())
        if n == 0:
            continue
        # the slab ends inside the last-but-one frame's addresses; the last frame lies wholly past the end
        at = (lay["offsets"].astype(np.int64) if lay["offsets"] is not None else np.arange(n) * lay["stride"]) + lay["data_off"]
        cut = int(at[max(n - 2, 0)]) + 28
        sel2 = None if sel is None else np.ones(n, np.uint8)       # both edge frames taken
        got, want, _ = run(cl, tables["a"], g["rules"], slab, n, lay, slab_len=cut, **{**kw, "sel": sel2, "mode": A.PERMISSIVE})
        if n >= 2:
            assert at[n - 1] >= cut and want["verdict"][n - 1] == A.PREFILTER and want["result"][n - 1] == 0
        assert at[max(n - 2, 0)] + 14 < cut < at[max(n - 2, 0)] + 33
    assert seen == ({A.NONE, A.PREFILTER, A.DENIED, A.FORWARD} if with_sel else {A.PREFILTER, A.DENIED, A.FORWARD})


def test_prefilter_reasons_and_quirks(cl, tables):
    """One frame for each prefilter reason (len 19, version 6, IHL 4,
    total_length 19); a non-IPv4 ethertype whose byte 14 is 0x45 is classified;
    IHL 6 is matched on bytes 26-33; an unknown dst_lport goes back to in_lport."""
    rules = A.golden("a")["rules"]
    src = np.array([0xD2000005] * 8 + [0x01010101, 0x0B000001], np.uint32)
    dst = np.array([0x6E000005] * 8 + [0x02020202, 0x02020202], np.uint32)
    rows = A.frames(src, dst, dmac5=np.array([1, 7, 1, 1, 1, 1, 1, 200, 1, 1]))
    rows[1, 12:14] = (0x86, 0xDD)
    rows[2, 14] = 0x46
    rows[3, 14] = 0x65
    rows[4, 14] = 0x44
    rows[5, 16:18] = (0, 19)
    length = np.full(10, 60, np.uint16)
    length[6], length[0] = 19, 20
    lay = dict(stride=64, offsets=None, data_off=0)
    for mode in (A.STRICT, A.PERMISSIVE):
        got, want, _ = run(cl, tables["a"], rules, rows.reshape(-1), 10, lay, mode=mode, swap=True, in_lport=3,
                           lports=(1, 3, 7), length=length)
        assert want["verdict"].tolist() == [3, 3, 3, 1, 1, 1, 1, 3, 3 if mode else 2, 2]
        assert want["tx_lport"].tolist() == [1, 7, 1, 255, 255, 255, 255, 3, 1 if mode else 255, 255]
        assert want["result"][:3].tolist() == [130 + 5 + 1] * 3 and want["result"][9] == 101 + A.DENY


def test_bin_of_feeds_bin_partition(cl, tables):
    g = A.golden("a")
    n = 1000
    rows = A.frames(g["psrc"][:n], g["pdst"][:n], dmac5=np.arange(n) % 9)
    rows[5::13, 14] = 0x60
    fr = to_frames(rows.reshape(-1), n, dict(stride=64, offsets=None, data_off=0))
    kw = dict(mode=A.PERMISSIVE, swap=False, in_lport=6, lports=(0, 2, 4))
    res = cl.acl_fwd(fr, tables["a"], **kw)
    want = A.acl_fwd_ref(rows.reshape(-1), n, g["rules"], stride=64, **kw)
    assert res["n_bins"] == want["n_bins"] == 7
    start, order = cl.bin_partition(res["bin_of"], res["n_bins"])
    torch.cuda.synchronize()
    bins = want["bin_of"].astype(np.int64)
    assert set(np.unique(bins)) == {0, 2, 4, 6, 7, 8}               # known ports, the echo port, denied, the rest
    assert np.array_equal(order.cpu().numpy(), np.argsort(bins, kind="stable"))
    assert np.array_equal(start.cpu().numpy()[:10], np.concatenate([[0], np.cumsum(np.bincount(bins, minlength=9))]))


def test_mirror_refresh_and_stats_accumulate(cl):
    """One table, one context: rules added after a build stay invisible to the
    device until the next build; the counters add up over calls."""
    src, dst = [0xD2000001, 0x01020304, 0xD2000002, 0x0B000001], [0x6E000001, 0x05060708, 0x6E000002, 0x6E000001]
    rows = A.frames(np.array(src * 16, np.uint32), np.array(dst * 16, np.uint32), dmac5=0)
    lay = dict(stride=64, offsets=None, data_off=0)
    kw = dict(mode=A.STRICT, swap=False, in_lport=0, lports=(0,))
    t = AclTable()
    assert t.build_raw() == -22
    fr = to_frames(rows.reshape(-1), 64, lay)
    out = {k: torch.full_like(v, 0x55) for k, v in alloc_acl_outputs(64, "cuda:0").items()}
    with pytest.raises(OSError) as e:                                # no image: -ENOENT, nothing written
        cl.acl_fwd(fr, t, acl=out, **kw)
    torch.cuda.synchronize()
    assert e.value.errno == 2 and all(bool((v == 0x55).all()) for v in out.values())
    t.add_init_rules()
    t.build()
    base = A.golden("a")["rules"]
    got1, _, res = run(cl, t, base, rows.reshape(-1), 64, lay, **kw)
    assert got1["verdict"][:4].tolist() == [A.FORWARD, A.DENIED, A.FORWARD, A.DENIED]
    t.clear()
    head = A.rules_of([(0xD2000002, 32, 0, 0, 1)])                   # shadows the later allow 210.0.0.2 -> 110.0.0.2
    tail = A.rules_of([(0x01020304, 32, 0x05060708, 32, 1)])         # shadows nothing: its packet matched no rule
    now = A.cat_rules(head, base, tail)
    t.add_many(now["src_addr"], now["src_msk"], now["dst_addr"], now["dst_msk"], now["deny"])
    got2, _, res = run(cl, t, base, rows.reshape(-1), 64, lay, acl=res, stats0=got1["stats"], **kw)   # no build yet
    assert np.array_equal(got2["result"], got1["result"]) and got2["stats"].tolist() == (2 * got1["stats"]).tolist()
    t.build()
    got3, _, _ = run(cl, t, now, rows.reshape(-1), 64, lay, acl=res, stats0=got2["stats"], **kw)
    assert got3["result"][:4].tolist() == [131 + 1 + 1, 4227 + A.DENY, 0 + A.DENY, 102 + A.DENY]
    cl.acl_fwd(to_frames(rows.reshape(-1), 0, lay), t, **kw)         # n == 0: nothing to launch
    torch.cuda.synchronize()
    t.close()


def test_a_table_at_the_rule_cap(cl):
    rules, psrc, pdst = A.big_rules()
    t = table(rules)
    rows = A.frames(psrc, pdst, dmac5=np.arange(512) % 3)
    slab, lay = A.layout(rows, "umem")
    for mode in (A.STRICT, A.PERMISSIVE):
        _, want, _ = run(cl, t, rules, slab, 512, lay, mode=mode, swap=True, in_lport=1, lports=(0, 1))
    assert set(np.unique(want["verdict"])) == {A.DENIED, A.FORWARD}
    t.close()

"""include/cndp_mqfwd.h on a machine without a GPU: the header compiles as C and
as C++, the library exports cndp_gpu_mq_create_fwd, NULL arguments are refused
before any device is touched, and the Python constants are the header's."""
import ctypes
import os
import re
import subprocess

import pytest

from cndp_amd import native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cndp_mqfwd.h")

USE = """
#include <string.h>
#include "cndp_mqfwd.h"
int use(cndp_gpu_ctx_t *c, struct cne_fib *f, cndp_acl_tbl_t *t, cndp_gpu_mq_t **q);
int use(cndp_gpu_ctx_t *c, struct cne_fib *f, cndp_acl_tbl_t *t, cndp_gpu_mq_t **q)
{
    struct cndp_mq_conf k;
    struct cndp_mq_fwd w;
    memset(&k, 0, sizeof(k));
    memset(&w, 0, sizeof(w));
    k.mode = CNDP_MQ_CFWD_L3FWD;
    k.lport = 3;
    w.fib = f;
    w.acl = t;
    w.acl_mode = CNDP_ACL_PERMISSIVE;
    w.acl_flags = CNDP_ACL_F_MAC_SWAP;
    w.lport_mask[3] = 1;
    return cndp_gpu_mq_create_fwd(c, &k, &w, q) + (int)sizeof(struct cndp_mq_fwd) + CNDP_MQ_EDGE_ECHO +
           CNDP_MQ_STAT_ACL_PERMIT;
}
"""


@pytest.mark.parametrize("lang,cc,std", [("c", "gcc", "-std=c11"), ("c++", "g++", "-std=c++17")])
def test_header_compiles(tmp_path, lang, cc, std):
    src = tmp_path / ("use.c" if lang == "c" else "use.cpp")
    src.write_text(USE)
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_symbol_exported():
    assert "cndp_gpu_mq_create_fwd" in N.exported_symbols()
    assert hasattr(N.lib(), "cndp_gpu_mq_create_fwd")
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "cndp_gpu_mq_create_fwd" in names
    assert not {"acl_dev_begin", "acl_dev_end"} & names     # the mirror's reader protocol stays internal


def test_null_arguments():
    L = N.lib()
    c, w, h = N.MqConf(), N.MqFwd(), ctypes.c_void_p()
    c.mode = N.CNDP_MQ_CFWD_FWD
    fake = ctypes.c_void_p(16)      # never dereferenced: every call below has a NULL among its arguments
    assert L.cndp_gpu_mq_create_fwd(None, ctypes.byref(c), ctypes.byref(w), ctypes.byref(h)) == -22
    assert L.cndp_gpu_mq_create_fwd(fake, None, ctypes.byref(w), ctypes.byref(h)) == -22
    assert L.cndp_gpu_mq_create_fwd(fake, ctypes.byref(c), None, ctypes.byref(h)) == -22
    assert L.cndp_gpu_mq_create_fwd(fake, ctypes.byref(c), ctypes.byref(w), None) == -22
    assert L.cndp_gpu_mq_create_fwd(None, None, None, None) == -22


def test_python_constants_match_header():
    txt = open(HEADER).read()
    defs = {m.group(1): int(m.group(2).rstrip("uU"), 0)
            for m in re.finditer(r"^#define\s+(CNDP_MQ_\w+)\s+(0[xX][0-9a-fA-F]+[uU]?|\d+[uU]?)\b", txt, re.M)}
    want = ["CNDP_MQ_CFWD_FWD", "CNDP_MQ_CFWD_L3FWD", "CNDP_MQ_ACL_FWD", "CNDP_MQ_EDGE_ECHO", "CNDP_MQ_EDGE_ACL_DENY",
            "CNDP_MQ_EDGE_ACL_PREFILTER", "CNDP_MQ_STAT_FORWARD", "CNDP_MQ_STAT_ECHO", "CNDP_MQ_STAT_ACL_PREFILTER",
            "CNDP_MQ_STAT_ACL_DENY", "CNDP_MQ_STAT_ACL_PERMIT"]
    assert sorted(defs) == sorted(want)
    for name in want:
        assert getattr(N, name) == defs[name], name
    assert (defs["CNDP_MQ_CFWD_FWD"], defs["CNDP_MQ_CFWD_L3FWD"], defs["CNDP_MQ_ACL_FWD"]) == (4, 5, 6)
    # struct cndp_mq_fwd: two pointers, two words, the 256-bit port map
    assert ctypes.sizeof(N.MqFwd) == 8 + 8 + 4 + 4 + 32
    assert N.MqFwd.lport_mask.offset == 24

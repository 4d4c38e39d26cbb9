"""ctypes binding of libcndp_gpu.so (the C-ABI declared in include/cndp_fib.h,
include/cndp_node.h, include/cndp_gpu.h, include/cndp_l4.h,
include/cndp_tcp.h, include/cndp_tcb.h, include/cndp_fwd.h, include/cndp_tx.h,
include/cndp_acl.h, include/cndp_cfwd.h, include/cndp_mqfwd.h,
include/cndp_mqcnet.h, include/cndp_mql4.h, include/cndp_mqtcp.h,
include/cndp_mqtx.h and include/cndp_mqtcb.h).

The library is built in-tree (cndp_amd/lib/libcndp_gpu.so, see build.py).
There is no fallback: if the shared object is missing, importing the
product API raises, so a test or bench can never silently run a CPU path.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, Union, c_char_p, c_int, c_uint8, c_uint16,
                    c_uint32, c_uint64, c_void_p)

HERE = os.path.dirname(os.path.abspath(__file__))
# CNDP_GPU_LIB: an alternative build of the same library (A/B timing experiments)
LIB_PATH = os.environ.get("CNDP_GPU_LIB") or os.path.join(HERE, "lib", "libcndp_gpu.so")

# cne_fib.h:34-38, :53-58, :60, :63-73 (+ CNE_FIB_LOOKUP_GPU)
CNE_FIB_DUMMY, CNE_FIB_DIR24_8, CNE_FIB_TRIE = 0, 1, 2
CNE_FIB_DIR24_8_1B, CNE_FIB_DIR24_8_2B, CNE_FIB_DIR24_8_4B, CNE_FIB_DIR24_8_8B = 0, 1, 2, 3
CNE_FIB_TRIE_2B, CNE_FIB_TRIE_4B, CNE_FIB_TRIE_8B = 1, 2, 3
(CNE_FIB_LOOKUP_DEFAULT, CNE_FIB_LOOKUP_DIR24_8_SCALAR_MACRO, CNE_FIB_LOOKUP_DIR24_8_SCALAR_INLINE,
 CNE_FIB_LOOKUP_DIR24_8_SCALAR_UNI, CNE_FIB_LOOKUP_DIR24_8_VECTOR_AVX512, CNE_FIB_LOOKUP_TRIE_SCALAR,
 CNE_FIB_LOOKUP_TRIE_VECTOR_AVX512, CNE_FIB_LOOKUP_GPU) = range(8)
CNE_FIB_MAXDEPTH = 32
CNE_FIB6_MAXDEPTH = 128

# cndp_gpu.h
CNDP_MODE_L3FWD, CNDP_MODE_CNET, CNDP_MODE_HASH = 0, 1, 2
CNDP_NH_INVALID = 0xFFFFFFFF
CNDP_EDGE_CLS_DROP = 0xFF
CNDP_RSS_KEY_LEN = 40
CNDP_RETA_MAX = 512
CNDP_BINS_MAX = 1024
CNDP_PART_BINS_MAX = 4096
CNDP_FRAMES_CACHED = 1
CNDP_TUNE_NT, CNDP_TUNE_UNROLL, CNDP_TUNE_BLOCKS_PER_CU, CNDP_TUNE_TILE, CNDP_TUNE_DIR16 = 1, 2, 3, 4, 5
CNDP_TUNE_CNET_TILE = 6
CNDP_TUNE_HOST_CHUNK = 7
CNDP_TUNE_RW_WB = 8
CNDP_TUNE_CNET_SPEC = 9
CNDP_TUNE_LOAD_NT = 10
CNDP_TUNE_SPEC_SCAN = 11
CNDP_STAT_CNET_WORKLIST, CNDP_STAT_CNET_UNIFORM, CNDP_STAT_SPEC_ERR = 1, 2, 3
CNDP_STAT_FIB_LDS = 4
CNDP_TUNE_MBUF_HASH = 12
CNDP_TUNE_CNET_FOLD = 13
CNDP_TUNE_SPEC_GRID = 14
CNDP_TUNE_SPEC_LISTS = 15
CNDP_TUNE_SPEC_TYPES = 16
CNDP_TUNE_STREAM_BAL = 17
CNDP_TUNE_FIB_LDS = 20
CNDP_TUNE_MQ_PCB_LDS = 21
CNDP_TUNE_SPEC_WAIT = 18
CNDP_TUNE_HOST_WINDOW = 19
CNDP_MQ_IP4_LOOKUP, CNDP_MQ_CNET, CNDP_MQ_MAC_SWAP, CNDP_MQ_IP4_REWRITE = 0, 1, 2, 3
CNDP_MQ_F_HASH, CNDP_MQ_F_NO_METADATA, CNDP_MQ_F_DEVICE_HEADERS, CNDP_MQ_F_RX_PARSE = 1, 2, 4, 8
CNDP_MQ_F_REWRITE = 16
CNDP_MQ_F_HOST_WRITEBACK = 1 << 5
CNDP_MQ_EDGE_NONE = 0xFFFF
CNDP_MQ_EDGE_CLS_DROP = 0xFFFE
CNDP_MQ_EDGE_LOOKUP_DROP = 0xFFFD
CNDP_MQ_STAT_BATCHES, CNDP_MQ_STAT_MBUFS = 1, 2
CNDP_MQ_NODE_PTYPE, CNDP_MQ_NODE_IP4, CNDP_MQ_NODE_IP6 = 0, 1, 2
CNDP_MBUF_EDGE_CLS_DROP = 0xFFFF

# l3fwd edges (node_ip4_api.h:28-34) and cnet edges (ip4_input_priv.h:26-31)
IP4_LOOKUP_NEXT_REWRITE, IP4_LOOKUP_NEXT_PKT_DROP = 0, 1
IP4_INPUT_NEXT_PKT_DROP, IP4_INPUT_NEXT_FORWARD, IP4_INPUT_NEXT_PROTO = 0, 1, 2

# cndp_l4.h
CNDP_PCB_MAX_ENTRIES = 4096
CNDP_PCB_NONE = 0xFFFFFFFF
CNDP_UDP_CHKSUM_FLAG = 0x0080
CNDP_L4_NODE_IP4_PROTO, CNDP_L4_NODE_UDP_INPUT = 0, 1
CNDP_L4_EDGE_NONE = 0xFF
CNDP_IP4_PROTO_DROP, CNDP_IP4_PROTO_TCP = 0, 2
CNDP_UDP_INPUT_PKT_DROP, CNDP_UDP_INPUT_CHNL_RECV, CNDP_UDP_INPUT_PKT_PUNT = 0, 1, 2
CNDP_L4_STAT_RECV, CNDP_L4_STAT_NOMATCH, CNDP_L4_STAT_CKSUM, CNDP_L4_STAT_PROTO_DROP = 0, 1, 2, 3

# cndp_tcp.h
CNDP_L4_NODE_TCP_INPUT = 2
CNDP_TCP_INPUT_PKT_DROP, CNDP_TCP_INPUT_SEGMENT, CNDP_TCP_INPUT_PKT_PUNT = 0, 1, 2
(CNDP_TCP_STAT_SEGMENT, CNDP_TCP_STAT_NOMATCH, CNDP_TCP_STAT_CKSUM, CNDP_TCP_STAT_BADOFF,
 CNDP_TCP_STAT_RSVD) = range(5)
CNDP_TCP_NSTATS = 5

# cndp_tcb.h
(CNDP_TCPS_FREE, CNDP_TCPS_CLOSED, CNDP_TCPS_LISTEN, CNDP_TCPS_SYN_SENT, CNDP_TCPS_SYN_RCVD, CNDP_TCPS_ESTABLISHED,
 CNDP_TCPS_CLOSE_WAIT, CNDP_TCPS_FIN_WAIT_1, CNDP_TCPS_CLOSING, CNDP_TCPS_LAST_ACK, CNDP_TCPS_FIN_WAIT_2,
 CNDP_TCPS_TIME_WAIT) = range(12)
CNDP_TCB_REASS_EMPTY = 1
CNDP_SEG_TS_PRESENT, CNDP_SEG_MSS_PRESENT, CNDP_SEG_WS_PRESENT, CNDP_SEG_SACK_PERMIT = 0x8000, 0x4000, 0x2000, 0x1000
CNDP_SEG_REQ_SCALE = 0x000F
(CNDP_TCPSEG_NONE, CNDP_TCPSEG_RESET, CNDP_TCPSEG_CLOSED, CNDP_TCPSEG_BADOPT, CNDP_TCPSEG_SLOW,
 CNDP_TCPSEG_PRED_ACK, CNDP_TCPSEG_PRED_DATA, CNDP_TCPSEG_PRED_NONE) = range(8)
CNDP_TCPSEG_NSTATS = 8
CNDP_TCPSEG_VERDICT, CNDP_TCPSEG_TS_UPDATE, CNDP_TCPSEG_FIRST = 0x0F, 0x40, 0x80

# cndp_tcpout.h
CNDP_TCBF_REQ_SCALE, CNDP_TCBF_RCVD_SCALE, CNDP_TCBF_REQ_TSTAMP, CNDP_TCBF_RCVD_TSTAMP = 0x01, 0x02, 0x04, 0x08
CNDP_TCPOUT_SEGMENT, CNDP_TCPOUT_RESPOND = 0, 1
(CNDP_TCPOUT_STAT_SENT, CNDP_TCPOUT_STAT_NOTSEL, CNDP_TCPOUT_STAT_NOPCB, CNDP_TCPOUT_STAT_NOLADDR,
 CNDP_TCPOUT_STAT_TOOBIG, CNDP_TCPOUT_STAT_RST_IN, CNDP_TCPOUT_STAT_MCAST, CNDP_TCPOUT_STAT_OPTS) = range(8)
CNDP_TCPOUT_NSTATS = 8

# cndp_fwd.h
CNDP_FWD_OBJS_MAX = 1 << 24
CNDP_FWD_NETIFS = 256
CNDP_FWD_NONE = 0xFFFFFFFF
CNDP_FWD_EDGE_PKT_DROP, CNDP_FWD_EDGE_ARP_REQUEST, CNDP_FWD_EDGE_OUTPUT = 0, 1, 2
CNDP_FWD_EDGE_NONE = 0xFFFF
CNDP_FWD_STAT_DIRECT, CNDP_FWD_STAT_GATEWAY, CNDP_FWD_STAT_ARP_REQUEST = 0, 1, 2

# cndp_tx.h
CNDP_TX_UDP, CNDP_TX_IP4 = 0, 1
CNDP_TX_EDGE_PKT_DROP, CNDP_TX_EDGE_ARP_REQUEST, CNDP_TX_EDGE_OUTPUT = 0, 1, 2
CNDP_TX_EDGE_NONE = 0xFFFF
(CNDP_TX_STAT_SENT, CNDP_TX_STAT_ARP_REQUEST, CNDP_TX_STAT_DROP_HEADROOM, CNDP_TX_STAT_DROP_NOROUTE,
 CNDP_TX_STAT_DROP_PROTO, CNDP_TX_STAT_CKSUM) = range(6)
CNDP_TX_NSTATS = 6

# cndp_acl.h
CNDP_ACL_MAX_RULES = 100000
CNDP_ACL_DENY_SIGNATURE = 0xF0000000
CNDP_ACL_INIT_RULES = 4226
CNDP_ACL_STRICT, CNDP_ACL_PERMISSIVE = 0, 1
CNDP_ACL_F_MAC_SWAP = 1
CNDP_ACL_NONE, CNDP_ACL_PREFILTER, CNDP_ACL_DENY, CNDP_ACL_FORWARD = range(4)
CNDP_ACL_LPORT_NONE = 0xFF
CNDP_ACL_STAT_PREFILTER_DROP, CNDP_ACL_STAT_DENY, CNDP_ACL_STAT_PERMIT = range(3)
CNDP_ACL_NSTATS = 3
# cndp_cfwd.h
CNDP_CFWD_FWD, CNDP_CFWD_L3FWD = 0, 1
CNDP_CFWD_DEFAULT_NH = 0xFFFFFFFFFFFF
CNDP_CFWD_MAX_ROUTES = 1 << 16
CNDP_CFWD_PORT_MAX = 0x7FFF
CNDP_CFWD_LPORT_NONE = 0xFFFF
CNDP_CFWD_STAT_FORWARD, CNDP_CFWD_STAT_ECHO = range(2)
CNDP_CFWD_NSTATS = 2
# cndp_mqfwd.h
CNDP_MQ_CFWD_FWD, CNDP_MQ_CFWD_L3FWD, CNDP_MQ_ACL_FWD = 4, 5, 6
CNDP_MQ_EDGE_ECHO = 0x0100
CNDP_MQ_EDGE_ACL_DENY = 0xFFFC
CNDP_MQ_EDGE_ACL_PREFILTER = 0xFFFB
(CNDP_MQ_STAT_FORWARD, CNDP_MQ_STAT_ECHO, CNDP_MQ_STAT_ACL_PREFILTER, CNDP_MQ_STAT_ACL_DENY,
 CNDP_MQ_STAT_ACL_PERMIT) = range(3, 8)
# cndp_mqcnet.h
CNDP_MQ_IP4_FORWARD = 7
CNDP_MQ_EDGE_FWD_GATEWAY = 0x0400
CNDP_MQ_EDGE_FWD_MASK = 0x01FF
CNDP_MQ_STAT_FWD_DIRECT, CNDP_MQ_STAT_FWD_GATEWAY, CNDP_MQ_STAT_FWD_ARP_REQUEST = range(8, 11)
# cndp_mql4.h
CNDP_MQ_UDP_INPUT = 8
CNDP_MQ_NODE_IP4_PROTO = 3
CNDP_MQ_NODE_UDP_INPUT = 4
CNDP_MQ_EDGE_L4_CKSUM = 0x0080
CNDP_MQ_EDGE_L4_MASK = 0xFF7F
(CNDP_MQ_STAT_L4_RECV, CNDP_MQ_STAT_L4_NOMATCH, CNDP_MQ_STAT_L4_CKSUM, CNDP_MQ_STAT_L4_PROTO_DROP,
 CNDP_MQ_STAT_L4_TCP, CNDP_MQ_STAT_L4_NOMD) = range(11, 17)
# cndp_mqtcp.h
CNDP_MQ_TCP_INPUT = 9
CNDP_MQ_NODE_TCP_INPUT = 5
CNDP_MQ_EDGE_TCP_IPOPT = 0x0040
CNDP_MQ_EDGE_TCP_MASK = 0xFF3F
(CNDP_MQ_STAT_TCP_SEGMENT, CNDP_MQ_STAT_TCP_NOMATCH, CNDP_MQ_STAT_TCP_CKSUM, CNDP_MQ_STAT_TCP_NOMD,
 CNDP_MQ_STAT_TCP_ADJUST, CNDP_MQ_STAT_TCP_SHORT, CNDP_MQ_STAT_TCP_BADOFF, CNDP_MQ_STAT_TCP_IPOPT) = range(17, 25)
# cndp_mqtx.h
CNDP_MQ_IP4_OUTPUT = 10
CNDP_MQ_EDGE_TX_MASK = 0x01FF
CNDP_MQ_EDGE_TX_CKSUM = 0x1000
CNDP_MQ_TX_CAUSE_NOMD, CNDP_MQ_TX_CAUSE_HEADROOM, CNDP_MQ_TX_CAUSE_NOROUTE, CNDP_MQ_TX_CAUSE_PROTO = 1, 2, 3, 4
(CNDP_MQ_STAT_TX_SENT, CNDP_MQ_STAT_TX_ARP_REQUEST, CNDP_MQ_STAT_TX_DROP_NOMD, CNDP_MQ_STAT_TX_DROP_HEADROOM,
 CNDP_MQ_STAT_TX_DROP_NOROUTE, CNDP_MQ_STAT_TX_DROP_PROTO, CNDP_MQ_STAT_TX_CKSUM) = range(25, 32)
# cndp_mqtcb.h
CNDP_MQ_TCP_SEGMENT = 11
(CNDP_MQ_STAT_TSEG_RESET, CNDP_MQ_STAT_TSEG_CLOSED, CNDP_MQ_STAT_TSEG_BADOPT, CNDP_MQ_STAT_TSEG_SLOW,
 CNDP_MQ_STAT_TSEG_PRED_ACK, CNDP_MQ_STAT_TSEG_PRED_DATA, CNDP_MQ_STAT_TSEG_PRED_NONE) = range(32, 39)


def CNDP_MQ_EDGE_TX_CAUSE(e: int) -> int:
    return (e >> 9) & 7


def CNDP_MQ_EDGE(node: int, e: int) -> int:
    return (node << 8) | e


def CNDP_L4_EDGE(node: int, e: int) -> int:
    return (node << 4) | e


MS_RSS_KEY = bytes.fromhex(
    "6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c6a42b73bbeac01fa")


class _Dir24(Structure):
    _fields_ = [("nh_sz", c_int), ("num_tbl8", c_uint32)]


class _ConfU(Union):
    _fields_ = [("dir24_8", _Dir24), ("trie", _Dir24)]


class FibConf(Structure):
    """struct cne_fib_conf (cne_fib.h:76-91)."""
    _anonymous_ = ("u",)
    _fields_ = [("type", c_int), ("default_nh", c_uint64), ("max_routes", c_int), ("u", _ConfU)]


class FibImage(Structure):
    _fields_ = [("nh_sz", c_uint32), ("tbl8_groups", c_uint32), ("tbl24", c_void_p),
                ("tbl8", c_void_p), ("def_nh", c_uint64)]


class FibNearInfo(Structure):
    """struct cndp_fib_near_info (cndp_fib.h)."""
    _fields_ = [("kib", c_uint32), ("cap_kib", c_uint32), ("fits", c_uint32), ("mid_used", c_uint32),
                ("mid_hwm", c_uint32), ("pages_used", c_uint32), ("page_hwm", c_uint32)]


class Batch(Structure):
    """struct cndp_batch (cndp_gpu.h)."""
    _fields_ = [("mode", c_uint32), ("n", c_uint32), ("slab", c_void_p), ("slab_len", c_uint64),
                ("stride", c_uint64), ("offsets", c_void_p), ("data_off", c_uint32),
                ("buf_len", c_uint32), ("nh", c_void_p), ("hash", c_void_p), ("queue", c_void_p),
                ("edge", c_void_p), ("bins", c_void_p), ("n_bins", c_uint32), ("ptype", c_void_p),
                ("rxmeta", c_void_p)]


class MqConf(Structure):
    """struct cndp_mq_conf (cndp_gpu.h)."""
    _fields_ = [("mode", c_uint32), ("flags", c_uint32), ("batch", c_uint32), ("depth", c_uint32),
                ("max_delay_us", c_uint32), ("stage_max", c_uint32), ("umem", c_void_p),
                ("lport", c_uint16), ("rsvd", c_uint16 * 3), ("metadata", c_void_p)]


class MqFwd(Structure):
    """struct cndp_mq_fwd (cndp_mqfwd.h)."""
    _fields_ = [("fib", c_void_p), ("acl", c_void_p), ("acl_mode", c_uint32), ("acl_flags", c_uint32),
                ("lport_mask", c_uint64 * 4)]


class PcbEntry(Structure):
    """struct cndp_pcb_entry (cndp_l4.h)."""
    _fields_ = [("laddr", c_uint32), ("faddr", c_uint32), ("lport", c_uint16), ("fport", c_uint16),
                ("opt_flag", c_uint16)]


class L4Io(Structure):
    """struct cndp_l4_io (cndp_l4.h)."""
    _fields_ = [("sel", c_void_p), ("l4edge", c_void_p), ("pcb", c_void_p), ("ports", c_void_p),
                ("payload_off", c_void_p), ("bin_of", c_void_p), ("n_bins", c_uint32),
                ("stats", c_void_p)]


class TcpIo(Structure):
    """struct cndp_tcp_io (cndp_tcp.h)."""
    _fields_ = [("sel", c_void_p), ("l4edge", c_void_p), ("pcb", c_void_p), ("ports", c_void_p),
                ("seg", c_void_p), ("bin_of", c_void_p), ("n_bins", c_uint32), ("stats", c_void_p)]


class Tcb(Structure):
    """struct cndp_tcb (cndp_tcb.h)."""
    _fields_ = [("rcv_nxt", c_uint32), ("snd_una", c_uint32), ("snd_nxt", c_uint32), ("snd_max", c_uint32),
                ("snd_wnd", c_uint32), ("snd_cwnd", c_uint32), ("ts_recent", c_uint32),
                ("last_ack_sent", c_uint32), ("rcv_space", c_uint32), ("max_mss", c_uint16), ("state", c_uint8),
                ("snd_scale", c_uint8), ("flags", c_uint8), ("rsvd", c_uint8 * 7)]


class TcpSegIo(Structure):
    """struct cndp_tcpseg_io (cndp_tcb.h)."""
    _fields_ = [("sel", c_void_p), ("l4edge", c_void_p), ("pcb", c_void_p), ("seg", c_void_p),
                ("opt", c_void_p), ("verdict", c_void_p), ("stats", c_void_p)]


class TcbTx(Structure):
    """struct cndp_tcb_tx (cndp_tcpout.h)."""
    _fields_ = [("tflags", c_uint8), ("req_recv_scale", c_uint8), ("rcv_scale", c_uint8), ("rsvd", c_uint8)]


class TcpOutIo(Structure):
    """struct cndp_tcpout_io (cndp_tcpout.h)."""
    _fields_ = [("sel", c_void_p), ("pcb", c_void_p), ("txseg", c_void_p), ("seg", c_void_p), ("verdict", c_void_p),
                ("rxmeta", c_void_p), ("snd", c_void_p), ("snd_len", c_uint64), ("src_off", c_void_p),
                ("len", c_void_p), ("faddr", c_void_p), ("laddr", c_void_p), ("taken", c_void_p),
                ("stats", c_void_p)]


class FwdArp(Structure):
    """struct cndp_fwd_arp (cndp_fwd.h)."""
    _fields_ = [("netif_idx", c_uint16), ("ha", c_uint8 * 6)]


class FwdRt(Structure):
    """struct cndp_fwd_rt (cndp_fwd.h)."""
    _fields_ = [("gateway", c_uint32), ("netif_idx", c_uint16)]


class FwdIo(Structure):
    """struct cndp_fwd_io (cndp_fwd.h)."""
    _fields_ = [("sel", c_void_p), ("fwd_edge", c_void_p), ("arp_idx", c_void_p), ("bin_of", c_void_p),
                ("n_bins", c_uint32), ("stats", c_void_p)]


class PcbTx(Structure):
    """struct cndp_pcb_tx (cndp_tx.h)."""
    _fields_ = [("tos", c_uint8), ("ttl", c_uint8), ("ip_proto", c_uint8)]


class TxIo(Structure):
    """struct cndp_tx_io (cndp_tx.h)."""
    _fields_ = [("sel", c_void_p), ("pcb", c_void_p), ("faddr", c_void_p), ("laddr", c_void_p),
                ("ports", c_void_p), ("len", c_void_p), ("tx_edge", c_void_p), ("bin_of", c_void_p),
                ("n_bins", c_uint32), ("stats", c_void_p)]


class AclRule(Structure):
    """struct cndp_acl_rule (cndp_acl.h)."""
    _fields_ = [("src_addr", c_uint32), ("dst_addr", c_uint32), ("src_msk", c_uint8), ("dst_msk", c_uint8),
                ("deny", c_uint8), ("rsvd", c_uint8)]


class AclIo(Structure):
    """struct cndp_acl_io (cndp_acl.h)."""
    _fields_ = [("sel", c_void_p), ("len", c_void_p), ("in_lport", c_uint32), ("lport_mask", c_uint64 * 4),
                ("result", c_void_p), ("verdict", c_void_p), ("tx_lport", c_void_p), ("bin_of", c_void_p),
                ("n_bins", c_uint32), ("stats", c_void_p)]


class CfwdIo(Structure):
    """struct cndp_cfwd_io (cndp_cfwd.h)."""
    _fields_ = [("sel", c_void_p), ("in_lport", c_uint32), ("lport_mask", c_uint64 * 4), ("nh", c_void_p),
                ("tx_lport", c_void_p), ("echoed", c_void_p), ("bin_of", c_void_p), ("n_bins", c_uint32),
                ("stats", c_void_p)]


class NativeLibraryMissing(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and return the native library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (no CPU fallback exists)")
    L = ctypes.CDLL(LIB_PATH)
    sig = {
        # cndp_fib.h
        "cne_fib_create": (c_void_p, [c_char_p, POINTER(FibConf)]),
        "cne_fib_free": (None, [c_void_p]),
        "cne_fib_add": (c_int, [c_void_p, c_uint32, c_uint8, c_uint64]),
        "cne_fib_delete": (c_int, [c_void_p, c_uint32, c_uint8]),
        "cne_fib_lookup_bulk": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
        "cne_fib_get_dp": (c_void_p, [c_void_p]),
        "cne_fib_get_rib": (c_void_p, [c_void_p]),
        "cne_fib_select_lookup": (c_int, [c_void_p, c_int]),
        "cne_fib6_create": (c_void_p, [c_char_p, POINTER(FibConf)]),
        "cne_fib6_free": (None, [c_void_p]),
        "cne_fib6_add": (c_int, [c_void_p, c_void_p, c_uint8, c_uint64]),
        "cne_fib6_delete": (c_int, [c_void_p, c_void_p, c_uint8]),
        "cne_fib6_lookup_bulk": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
        "cne_fib6_get_dp": (c_void_p, [c_void_p]),
        "cne_fib6_get_rib": (c_void_p, [c_void_p]),
        "cne_fib6_select_lookup": (c_int, [c_void_p, c_int]),
        "cndp_fib_image": (c_int, [c_void_p, POINTER(FibImage)]),
        "cndp_fib6_image": (c_int, [c_void_p, POINTER(FibImage)]),
        "cndp_fib_sync": (c_int, [c_void_p, c_void_p]),
        "cndp_fib6_sync": (c_int, [c_void_p, c_void_p]),
        "cndp_fib_lookup_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
        "cndp_fib6_lookup_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
        "cndp_fib_stats": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
        "cndp_fib6_stats": (c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]),
        "cndp_fib_sync_stats": (c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
        "cndp_fib6_sync_stats": (c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
        "cndp_fib_near_refresh": (c_int, [c_void_p]),
        "cndp_fib_near_info": (c_int, [c_void_p, POINTER(FibNearInfo)]),
        "cndp_fib_near_lookup": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
        # cndp_node.h
        "cne_node_ip4_route_add": (c_int, [c_uint32, c_uint8, c_uint16, c_int]),
        "cne_node_ip4_rewrite_add": (c_int, [c_uint16, c_void_p, c_uint8, c_uint16]),
        "ip4_rewrite_set_next": (c_int, [c_uint16, c_uint16]),
        "cne_node_ip4_add_input": (c_int, [c_void_p, c_uint32, c_uint8, c_uint32]),
        "cne_node_ip6_add_input": (c_int, [c_void_p, c_void_p, c_uint8, c_uint32]),
        "cndp_node_ip4_lookup_init": (c_int, []),
        "cndp_node_ip4_lookup_fib": (c_void_p, []),
        "cndp_node_ip4_lookup_fini": (None, []),
        "cndp_node_ip4_rewrite_get": (c_int, [c_uint16, c_void_p, POINTER(c_uint16), POINTER(c_uint16),
                                              POINTER(c_uint16)]),
        "cndp_node_ip4_rewrite_reset": (None, []),
        "cndp_node_gpu_umem_add": (c_int, [c_void_p, c_uint64]),
        "cndp_node_gpu_umem_get": (c_int, [c_uint32, POINTER(c_void_p), POINTER(c_uint64)]),
        "cndp_node_gpu_umem_reset": (None, []),
        # cndp_gpu.h
        "cndp_gpu_init": (c_int, [c_int, POINTER(c_void_p)]),
        "cndp_gpu_fini": (None, [c_void_p]),
        "cndp_gpu_device": (c_int, [c_void_p]),
        "cndp_gpu_set_rss": (c_int, [c_void_p, c_char_p, c_uint32, c_void_p, c_uint32, c_uint32]),
        "cndp_gpu_set_fib": (c_int, [c_void_p, c_void_p, c_void_p]),
        "cndp_gpu_classify": (c_int, [c_void_p, POINTER(Batch), c_void_p]),
        "cndp_gpu_stream_release": (c_int, [c_void_p, c_void_p]),
        "cndp_gpu_classify_host": (c_int, [c_void_p, POINTER(Batch)]),
        "cndp_gpu_host_register": (c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_void_p)]),
        "cndp_gpu_host_unregister": (c_int, [c_void_p, c_void_p]),
        "cndp_gpu_frames_alloc": (c_int, [c_int, c_uint64, c_uint32, POINTER(c_void_p)]),
        "cndp_gpu_frames_free": (c_int, [c_void_p]),
        "cndp_gpu_l3fwd_mbufs": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p]),
        "cndp_gpu_ip4_rewrite_set_next": (c_int, [c_void_p, c_uint16, c_uint16]),
        "cndp_gpu_ip4_rewrite_add": (c_int, [c_void_p, c_uint16, c_void_p, c_uint8, c_uint16]),
        "cndp_gpu_ip4_rewrite": (c_int, [c_void_p, POINTER(Batch), c_uint32, c_void_p, c_void_p]),
        "cndp_gpu_mac_swap": (c_int, [c_void_p, POINTER(Batch), c_void_p]),
        "cndp_gpu_classify_rewrite": (c_int, [c_void_p, POINTER(Batch), c_uint32, c_void_p, c_void_p]),
        "cndp_gpu_bin_partition": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_void_p,
                                           c_void_p, c_void_p]),
        "cndp_gpu_bin_ids": (c_int, [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32,
                                     c_uint32, c_void_p, c_void_p]),
        "cndp_gpu_set_tuning": (c_int, [c_void_p, c_int, c_int]),
        "cndp_gpu_mq_create": (c_int, [c_void_p, POINTER(MqConf), POINTER(c_void_p)]),
        "cndp_gpu_mq_create_fwd": (c_int, [c_void_p, POINTER(MqConf), POINTER(MqFwd), POINTER(c_void_p)]),
        "cndp_gpu_mq_create_ip4_forward": (c_int, [c_void_p, POINTER(MqConf), c_void_p, POINTER(c_void_p)]),
        "cndp_gpu_mq_create_udp_input": (c_int, [c_void_p, POINTER(MqConf), c_void_p, POINTER(c_void_p)]),
        "cndp_gpu_mq_free": (None, [c_void_p]),
        "cndp_gpu_mq_submit": (c_int, [c_void_p, c_void_p, c_uint32]),
        "cndp_gpu_mq_flush": (c_int, [c_void_p]),
        "cndp_gpu_mq_poll": (c_int, [c_void_p, c_void_p, c_void_p, c_uint32]),
        "cndp_gpu_mq_wait": (c_int, [c_void_p]),
        "cndp_gpu_mq_pending": (c_uint32, [c_void_p]),
        "cndp_gpu_mq_stat": (ctypes.c_int64, [c_void_p, c_int]),
        "cndp_gpu_get_stat": (ctypes.c_int64, [c_void_p, c_int]),
        "cndp_gpu_version": (c_char_p, []),
        # cndp_l4.h
        "cndp_pcb_create": (c_int, [c_uint32, POINTER(c_void_p)]),
        "cndp_pcb_free": (None, [c_void_p]),
        "cndp_pcb_add": (c_int, [c_void_p, POINTER(PcbEntry)]),
        "cndp_pcb_del": (c_int, [c_void_p, c_uint32]),
        "cndp_pcb_set_flags": (c_int, [c_void_p, c_int, c_int]),
        "cndp_pcb_count": (c_int, [c_void_p]),
        "cndp_pcb_lookup": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
        "cndp_gpu_udp_input": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(L4Io), c_void_p]),
        # cndp_tcp.h
        "cndp_pcb_lookup_indexed": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
        "cndp_gpu_tcp_input": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(TcpIo), c_void_p]),
        # cndp_tcb.h
        "cndp_tcb_tbl_create": (c_int, [c_void_p, POINTER(c_void_p)]),
        "cndp_tcb_tbl_destroy": (None, [c_void_p]),
        "cndp_tcb_set": (c_int, [c_void_p, c_uint32, POINTER(Tcb)]),
        "cndp_tcb_clear": (c_int, [c_void_p, c_uint32]),
        "cndp_tcb_get": (c_int, [c_void_p, c_uint32, POINTER(Tcb)]),
        "cndp_gpu_tcp_segment": (c_int, [c_void_p, c_void_p, POINTER(Batch), POINTER(TcpSegIo), c_uint32, c_void_p]),
        "cndp_tcp_segment_host": (c_int, [c_void_p, c_uint32, POINTER(Batch), POINTER(TcpSegIo)]),
        # cndp_tcpout.h
        "cndp_tcb_tx_set": (c_int, [c_void_p, c_uint32, POINTER(TcbTx)]),
        "cndp_tcb_tx_get": (c_int, [c_void_p, c_uint32, POINTER(TcbTx)]),
        "cndp_tcp_output_host": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_uint64, c_uint64, c_void_p,
                                         c_uint32, c_uint32, POINTER(TcpOutIo)]),
        "cndp_tcp_send_optlen": (c_uint32, [c_uint8, c_uint8]),
        # cndp_fwd.h
        "cndp_fwd_create": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, POINTER(c_void_p)]),
        "cndp_fwd_free": (None, [c_void_p]),
        "cndp_fwd_arp_set": (c_int, [c_void_p, c_uint32, POINTER(FwdArp)]),
        "cndp_fwd_arp_clear": (c_int, [c_void_p, c_uint32]),
        "cndp_fwd_rt_set": (c_int, [c_void_p, c_uint32, POINTER(FwdRt)]),
        "cndp_fwd_rt_clear": (c_int, [c_void_p, c_uint32]),
        "cndp_fwd_netif_set": (c_int, [c_void_p, c_uint32, c_void_p]),
        "cndp_fwd_max_netif": (c_int, [c_void_p]),
        "cndp_fwd_lookup": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p]),
        "cndp_gpu_ip4_forward": (c_int, [c_void_p, c_void_p, POINTER(Batch), c_uint32, POINTER(FwdIo), c_void_p]),
        # cndp_mqcnet.h
        "cndp_fwd_node_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p]),
        # cndp_mql4.h
        "cndp_udp_input_node_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p]),
        "cndp_pcb_user_set": (c_int, [c_void_p, c_uint32, ctypes.c_uint64]),
        "cndp_pcb_user_get": (c_int, [c_void_p, c_uint32, POINTER(ctypes.c_uint64)]),
        # cndp_mqtcp.h
        "cndp_gpu_mq_create_tcp_input": (c_int, [c_void_p, POINTER(MqConf), c_void_p, POINTER(c_void_p)]),
        "cndp_gpu_mq_poll_tcp": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]),
        "cndp_tcp_input_node_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32,
                                             c_void_p]),
        # cndp_mqtcb.h
        "cndp_gpu_mq_create_tcp_segment": (c_int, [c_void_p, POINTER(MqConf), c_void_p, c_void_p, POINTER(c_void_p)]),
        "cndp_gpu_mq_tcp_now": (c_int, [c_void_p, c_uint32]),
        "cndp_gpu_mq_poll_tcpseg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]),
        "cndp_tcp_segment_node_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
        # cndp_mqtx.h
        "cndp_gpu_mq_create_ip4_output": (c_int, [c_void_p, POINTER(MqConf), c_void_p, c_void_p, c_uint32,
                                                  POINTER(c_void_p)]),
        "cndp_ip4_output_node_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_void_p,
                                              c_uint32, c_void_p]),
        # cndp_tx.h
        "cndp_pcb_tx_set": (c_int, [c_void_p, c_uint32, POINTER(PcbTx)]),
        "cndp_pcb_tx_get": (c_int, [c_void_p, c_uint32, POINTER(PcbTx)]),
        "cndp_fwd_netif_ident_set": (c_int, [c_void_p, c_uint32, c_uint16]),
        "cndp_fwd_netif_ident_get": (c_int, [c_void_p, c_uint32, POINTER(c_uint16)]),
        "cndp_gpu_ip4_output": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(Batch), c_uint32, POINTER(TxIo),
                                        c_void_p]),
        "cndp_tx_output_host": (c_int, [c_void_p, c_void_p, c_uint32, c_void_p, c_uint64, c_uint64, c_void_p,
                                        c_uint32, c_uint32, POINTER(TxIo)]),
        # cndp_acl.h
        "cndp_acl_tbl_create": (c_int, [POINTER(c_void_p)]),
        "cndp_acl_tbl_destroy": (None, [c_void_p]),
        "cndp_acl_add": (c_int, [c_void_p, POINTER(AclRule)]),
        "cndp_acl_clear": (c_int, [c_void_p]),
        "cndp_acl_count": (c_int, [c_void_p]),
        "cndp_acl_get": (c_int, [c_void_p, c_uint32, POINTER(AclRule)]),
        "cndp_acl_add_init_rules": (c_int, [c_void_p]),
        "cndp_acl_build": (c_int, [c_void_p]),
        "cndp_gpu_acl_fwd": (c_int, [c_void_p, c_void_p, POINTER(Batch), c_uint32, c_uint32, POINTER(AclIo), c_void_p]),
        "cndp_acl_classify_host": (c_int, [c_void_p, POINTER(Batch), c_uint32, c_uint32, POINTER(AclIo)]),
        # cndp_cfwd.h
        "cndp_cfwd_fib_create": (c_void_p, [c_char_p]),
        "cndp_cfwd_nexthop": (c_uint64, [c_void_p, c_uint16]),
        "cndp_cfwd_route_add": (c_int, [c_void_p, c_uint32, c_uint8, c_void_p, c_uint16]),
        "cndp_gpu_cfwd": (c_int, [c_void_p, c_void_p, POINTER(Batch), c_uint32, POINTER(CfwdIo), c_void_p]),
        "cndp_cfwd_host": (c_int, [c_void_p, POINTER(Batch), c_uint32, POINTER(CfwdIo)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def exported_symbols():
    """Names the C-ABI headers declare (checked against the .so by tests)."""
    import re
    names = []
    inc = os.path.join(os.path.dirname(HERE), "include")
    for h in ("cndp_fib.h", "cndp_node.h", "cndp_gpu.h", "cndp_mqfwd.h", "cndp_mqcnet.h", "cndp_mql4.h", "cndp_mqtcp.h",
              "cndp_mqtx.h", "cndp_mqtcb.h"):
        with open(os.path.join(inc, h)) as f:
            txt = f.read()
        names += re.findall(r"^[A-Za-z_][\w \*]*?\b((?:cne|cndp|ip4)_\w+)\s*\(", txt, re.M)
    return sorted(set(n for n in names if not n.endswith("_fn_t")))


def l4_exported_symbols(header: str = "cndp_l4.h"):
    """Names include/cndp_l4.h (or another header of include/) declares."""
    import re
    with open(os.path.join(os.path.dirname(HERE), "include", header)) as f:
        txt = f.read()
    return sorted(set(re.findall(r"^[A-Za-z_][\w \*]*?\b(cndp_\w+)\s*\(", txt, re.M)))


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise OSError(-rc, f"{what} failed: {os.strerror(-rc)}")
    return rc

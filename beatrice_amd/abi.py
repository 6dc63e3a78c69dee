"""ctypes binding of the C-ABI in include/beatrice_gpu.h (libbeatrice_gpu.so).

This is the Python-side caller of the drop-in boundary, used by tests/ and bench.py;
the production caller is the C++ adapter in beatrice_amd/host/. There is no CPU
fallback: if the HIP library is missing or no GPU is visible, Context() raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BT_LIB_PATH") or os.path.join(HERE, "libbeatrice_gpu.so")

BT_REC_BYTES = 96
ABI_VERSION = 2     # include/beatrice_gpu.h BT_ABI_VERSION this binding is written against
BT_MAX_FILTERS = 64

# FilterType order (reference include/beatrice/PacketFilter.hpp:17-24)
BPF, PROTOCOL, IP_RANGE, PORT_RANGE, PAYLOAD, CUSTOM = range(6)
DECIDE_PASS, DECIDE_REJECT, DECIDE_THROW, DECIDE_HOST = range(4)
KINDS = ["TRUE", "FALSE", "BPF", "PROTO_EQ", "PROTO_NZ", "IP_MASK", "PORT", "IP_THROW", "PORT_THROW", "HOST",
         "PAYLOAD"]

L_ETH, L_VLAN0, L_VLAN1, L_IPV4, L_IPV6, L_TCP, L_UDP, L_ICMP = (1 << i for i in range(8))
# bt_rec.detect_code: reference ProtocolDetector::detectProtocol names (ProtocolRegistry.cpp:353-388)
DETECT_NAMES = ("unknown", "", "ethernet", "tcp", "udp", "icmp")

# numpy view of bt_rec (96 B, include/beatrice_gpu.h)
REC_DTYPE = np.dtype({
    "names": ["eth_dst", "eth_src", "ethertype", "pkt_len", "vlan_tpid", "vlan_tci", "present", "ok",
              "l3_off", "l4_off", "l3", "l4", "detect_code", "detect_is", "detect_is2", "reserved"],
    "formats": [("u1", 6), ("u1", 6), "<u2", "<u2", ("<u2", 2), ("<u2", 2), "u1", "u1", "u1", "u1",
                ("u1", 40), ("u1", 20), "u1", "u1", "u1", ("u1", 5)],
    "offsets": [0, 6, 12, 14, 16, 20, 24, 25, 26, 27, 28, 68, 88, 89, 90, 91],
    "itemsize": 96,
})


class BtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"beatrice_gpu error {code}: {msg}")
        self.code = code


class FilterDesc(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("expression", ctypes.c_char_p), ("enabled", ctypes.c_int32),
                ("priority", ctypes.c_int32), ("has_custom_func", ctypes.c_int32)]


class FilterSlot(ctypes.Structure):
    _fields_ = [("source_index", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("a", ctypes.c_uint32),
                ("b", ctypes.c_uint32), ("throw_kind", ctypes.c_int32)]


class Opts(ctypes.Structure):
    _fields_ = [("host_chunk_packets", ctypes.c_uint32), ("host_chunk_bytes", ctypes.c_uint32),
                ("grid_waves", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("host_threads", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 3)]


OPT_NO_PREFETCH = 0x1
OPT_TILE_BLOCKED = 0x2
OPT_RECORDS_AOS = 0x4
OPT_GRAPH = 0x8
OPT_RECORDS_PLANES = 0x10
OPT_NT_STORES = 0x20
OPT_NT_LOADS = 0x40
OPT_CACHE_DEFAULT = 0x80
OPT_SPIN_SYNC = 0x100
OPT_PAYLOAD_HOST = 0x200
OPT_WIDE_NEVER = 0x400
OPT_WIDE_ALWAYS = 0x800
OPT_PIPELINE = 0x2000
OPT_GROUP_SHARED_DEVICE = 0x4000
OPT_NO_LEAN_PCIE = 0x8000
OPT_MAPPED_GATHER_SPARSE = 0x10000
OPT_NO_LEAN_HOST = 0x20000
OPT_PAYLOAD_DFA = 0x40000
OPT_PAYLOAD_EXTENDED = 0x80000   # PAYLOAD slots: \b \B, POSIX classes and wide DFAs on the GPU too
# bt_payload_dfa_compile_ex flags
DFA_NO_PAIRS = 0x1
DFA_NO_BITPAR = 0x2
DFA_EXTENDED = 0x4
TIME_KERNEL_EVENTS = 0x1
TIME_PIPELINED = 0x2


DESC_PACKED, DESC_XDP = 0, 1


class Batch(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("desc", ctypes.c_void_p), ("stride", ctypes.c_uint32),
                ("n", ctypes.c_uint32), ("bytes", ctypes.c_uint64), ("desc_format", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class Outputs(ctypes.Structure):
    _fields_ = [("records", ctypes.c_void_p), ("n_cap", ctypes.c_uint32), ("verdict", ctypes.c_void_p),
                ("decide", ctypes.c_void_p), ("pass_idx", ctypes.c_void_p), ("n_pass", ctypes.c_void_p)]


class PackOpts(ctypes.Structure):
    """bt_pack_opts (include/beatrice_gpu.h)."""
    _fields_ = [("lead", ctypes.c_uint32), ("snap", ctypes.c_uint32), ("align", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class PackOut(ctypes.Structure):
    """bt_pack_out: device-visible pointers."""
    _fields_ = [("bytes", ctypes.c_void_p), ("cap", ctypes.c_uint64), ("desc", ctypes.c_void_p),
                ("total", ctypes.c_void_p), ("n_packed", ctypes.c_void_p)]


TALLY_STOP_AT_THROW = 0x1   # count only the packets before the first DECIDE_THROW
TALLY_ACCUMULATE = 0x2      # add to the counts *out already holds
LAYER_NAMES = ("ethernet", "vlan0", "vlan1", "ipv4", "ipv6", "tcp", "udp", "icmp")   # bit k of present / ok


class Tally(ctypes.Structure):
    """bt_tally (2,304 B): bt_tally_device's counts of a device-resident batch."""
    _fields_ = [("n", ctypes.c_uint64), ("scanned", ctypes.c_uint64), ("first_throw", ctypes.c_uint64),
                ("first_host", ctypes.c_uint64), ("first_throw_slot", ctypes.c_uint32),
                ("first_host_slot", ctypes.c_uint32), ("code", ctypes.c_uint64 * 4),
                ("slot", (ctypes.c_uint64 * 64) * 4), ("bytes", ctypes.c_uint64 * 4),
                ("layer_present", ctypes.c_uint64 * 8), ("layer_ok", ctypes.c_uint64 * 8),
                ("reserved", ctypes.c_uint64 * 3)]

    def as_dict(self) -> dict:
        """Plain ints and lists; slot[code][s]."""
        out = {k: int(getattr(self, k)) for k in ("n", "scanned", "first_throw", "first_host", "first_throw_slot",
                                                  "first_host_slot")}
        for k in ("code", "bytes", "layer_present", "layer_ok", "reserved"):
            out[k] = [int(x) for x in getattr(self, k)]
        out["slot"] = [[int(x) for x in row] for row in self.slot]
        return out

    @classmethod
    def from_bytes(cls, buf) -> "Tally":
        """The struct held in 2,304 downloaded bytes."""
        return cls.from_buffer_copy(bytes(bytearray(_byte_view(buf)[:ctypes.sizeof(cls)])))


FANOUT_MAX_QUEUES = 64
FANOUT_KEY_USER = 0x1        # use FanoutOpts.key; else the RSS verification key
FANOUT_KEY_SYMMETRIC = 0x2   # the 0x6d5a-repeated key: both directions of a connection hash alike
FANOUT_RETA_USER = 0x4       # use FanoutOpts.reta (every entry < queues); else reta[i] = i % queues
FANOUT_L3_ONLY = 0x8         # never hash ports
FLOW_NONE, FLOW_V4, FLOW_V4_L4, FLOW_V6, FLOW_V6_L4 = range(5)
FLOW_NAMES = ("none", "ipv4", "ipv4_l4", "ipv6", "ipv6_l4")


class FanoutOpts(ctypes.Structure):
    """bt_fanout_opts: queues (1..64), FANOUT_* flags, a 40-byte key and a 128-entry indirection table."""
    _fields_ = [("queues", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("key", ctypes.c_uint8 * 40),
                ("reta", ctypes.c_uint8 * 128)]

    @classmethod
    def make(cls, queues: int, flags: int = 0, key=None, reta=None) -> "FanoutOpts":
        """key (40 bytes) sets FANOUT_KEY_USER, reta (128 entries) FANOUT_RETA_USER."""
        o = cls(queues, flags)
        if key is not None:
            o.flags |= FANOUT_KEY_USER
            o.key[:] = list(bytes(key))
        if reta is not None:
            o.flags |= FANOUT_RETA_USER
            o.reta[:] = [int(x) for x in reta]
        return o


class FanoutResult(ctypes.Structure):
    """bt_fanout_result (808 B): bt_flow_fanout_device's queue ranges, byte sums and class counts."""
    _fields_ = [("n", ctypes.c_uint32), ("n_selected", ctypes.c_uint32), ("start", ctypes.c_uint32 * 65),
                ("pad0", ctypes.c_uint32), ("bytes", ctypes.c_uint64 * 64), ("klass", ctypes.c_uint32 * 5),
                ("pad1", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        """Plain ints and lists."""
        out = {k: int(getattr(self, k)) for k in ("n", "n_selected", "pad0", "pad1")}
        for k in ("start", "bytes", "klass"):
            out[k] = [int(x) for x in getattr(self, k)]
        return out

    @classmethod
    def from_bytes(cls, buf) -> "FanoutResult":
        """The struct held in 808 downloaded bytes."""
        return cls.from_buffer_copy(bytes(bytearray(_byte_view(buf)[:ctypes.sizeof(cls)])))


class FanoutOut(ctypes.Structure):
    """bt_fanout_out: device-visible pointers; all but result optional."""
    _fields_ = [("hash", ctypes.c_void_p), ("queue", ctypes.c_void_p), ("idx", ctypes.c_void_p),
                ("select_q", ctypes.c_void_p), ("result", ctypes.c_void_p)]


def flow_hash_host(frame, opts: "FanoutOpts") -> tuple:
    """bt_flow_hash_host (host only): (hash, class, queue) of one frame (bytes or a uint8 array)."""
    a = _byte_view(frame)
    keep = a if len(a) else np.zeros(1, np.uint8)
    h, k, q = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    _check(lib().bt_flow_hash_host(keep.ctypes.data, len(a), ctypes.byref(opts), ctypes.byref(h), ctypes.byref(k),
                                   ctypes.byref(q)))
    return h.value, k.value, q.value


FLOWTAB_L3_ONLY = 0x1          # as FANOUT_L3_ONLY: never key on ports
FLOWTAB_BIDIRECTIONAL = 0x2    # both directions of a conversation are one flow
FLOW_ID_UNSELECTED = 0xFFFFFFFF   # packet not in `select`
FLOW_ID_NONE = 0xFFFFFFFE         # selected, FLOW_NONE: no key, not in the table
FLOW_ID_OVERFLOW = 0xFFFFFFFD     # selected, keyed, the table was full

# numpy view of bt_flow_rec (80 B): key in wire order (v4 src dst [sport dport]; v6 src dst [sport dport])
FlowRec = np.dtype({
    "names": ["key", "klass", "pad", "first", "last", "packets", "bytes", "reserved"],
    "formats": [("u1", 36), "u1", ("u1", 3), "<u4", "<u4", ("<u4", 2), ("<u8", 2), "<u8"],
    "offsets": [0, 36, 37, 40, 44, 48, 56, 72],
    "itemsize": 80,
})


class FlowTableOpts(ctypes.Structure):
    """bt_flow_table_opts: FLOWTAB_* flags, slots (a power of two >= 128; 0 = the smallest >= 2 n), flow_cap."""
    _fields_ = [("flags", ctypes.c_uint32), ("slots", ctypes.c_uint32), ("flow_cap", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class FlowTableResult(ctypes.Structure):
    """bt_flow_table_result (72 B): the counts of a flow table call."""
    _fields_ = [("n", ctypes.c_uint32), ("n_selected", ctypes.c_uint32), ("n_flows", ctypes.c_uint32),
                ("n_written", ctypes.c_uint32), ("none_packets", ctypes.c_uint32), ("overflow_packets", ctypes.c_uint32),
                ("slots", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("klass_flows", ctypes.c_uint32 * 5),
                ("pad", ctypes.c_uint32), ("none_bytes", ctypes.c_uint64), ("keyed_bytes", ctypes.c_uint64)]

    def as_dict(self) -> dict:
        """Plain ints and lists."""
        out = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "klass_flows"}
        out["klass_flows"] = [int(x) for x in self.klass_flows]
        return out

    @classmethod
    def from_bytes(cls, buf) -> "FlowTableResult":
        """The struct held in 72 downloaded bytes."""
        return cls.from_buffer_copy(bytes(bytearray(_byte_view(buf)[:ctypes.sizeof(cls)])))


class FlowTableOut(ctypes.Structure):
    """bt_flow_table_out: device-visible pointers; result is required."""
    _fields_ = [("flow_id", ctypes.c_void_p), ("flows", ctypes.c_void_p), ("result", ctypes.c_void_p)]


def flow_table_scratch_bytes(n: int, slots: int = 0) -> int:
    """bt_flow_table_scratch_bytes (host only): the scratch a flow table call over n packets needs."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_table_scratch_bytes(n, slots, ctypes.byref(b)))
    return b.value


def flow_table_host(data, desc, opts: "FlowTableOpts", select=None, nbytes=None) -> tuple:
    """bt_flow_table_host (host only): the flow table of the frames desc (packed descriptors) lists
    in `data`, of which `nbytes` (default: all) are readable. select: verdict-layout words or
    None. Returns (flow_id [n] u32, flows [n_written] FlowRec, result dict)."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    sel = None if select is None else np.ascontiguousarray(select, np.uint64)
    flow_id = np.zeros(max(1, n), np.uint32)
    flows = np.zeros(max(1, opts.flow_cap), FlowRec)
    res = FlowTableResult()
    _check(lib().bt_flow_table_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, d.ctypes.data if n else None, n,
                                    sel.ctypes.data if sel is not None and len(sel) else None, ctypes.byref(opts),
                                    flow_id.ctypes.data, flows.ctypes.data if opts.flow_cap else None, ctypes.byref(res)))
    return flow_id[:n], flows[:res.n_written], res.as_dict()


FLOW_ID_EXPIRED = 0xFFFFFFFB      # remap[] of an expire: the flow was removed
FLOW_TRACK_MAGIC = 0x4B525446

# numpy view of bt_flow_track_rec (104 B): record f of a tracker state is flow number f
FlowTrackRec = np.dtype({
    "names": ["key", "klass", "pad", "first_batch", "last_batch", "first", "last", "packets", "bytes", "first_ts", "last_ts"],
    "formats": [("u1", 36), "u1", ("u1", 3), "<u4", "<u4", "<u4", "<u4", ("<u8", 2), ("<u8", 2), "<u8", "<u8"],
    "offsets": [0, 36, 37, 40, 44, 48, 52, 56, 72, 88, 96],
    "itemsize": 104,
})


class _Counts(ctypes.Structure):
    def as_dict(self) -> dict:
        """Plain ints (arrays as lists)."""
        return {k: (int(v) if isinstance(v := getattr(self, k), int) else [int(x) for x in v]) for k, _ in self._fields_}

    @classmethod
    def from_bytes(cls, buf):
        """The struct held in downloaded bytes."""
        return cls.from_buffer_copy(bytes(bytearray(_byte_view(buf)[:ctypes.sizeof(cls)])))


class FlowTrackHdr(_Counts):
    """bt_flow_track_hdr (128 B): the head of a tracker state."""
    _fields_ = [("magic", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("flow_cap", ctypes.c_uint32), ("slots", ctypes.c_uint32),
                ("n_flows", ctypes.c_uint32), ("seq", ctypes.c_uint32),
                ("selected_packets", ctypes.c_uint64), ("keyed_packets", ctypes.c_uint64), ("none_packets", ctypes.c_uint64),
                ("overflow_packets", ctypes.c_uint64), ("selected_bytes", ctypes.c_uint64), ("keyed_bytes", ctypes.c_uint64),
                ("none_bytes", ctypes.c_uint64), ("overflow_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 5)]


class FlowTrackOpts(ctypes.Structure):
    """bt_flow_track_opts: FLOWTAB_* flags, flow_cap, slots (0 = the smallest power of two >= max(128, 2 flow_cap))."""
    _fields_ = [("flags", ctypes.c_uint32), ("flow_cap", ctypes.c_uint32), ("slots", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FlowTrackSizes(_Counts):
    """bt_flow_track_sizes: the size of a tracker state and the offsets of its parts."""
    _fields_ = [("total", ctypes.c_uint64), ("header", ctypes.c_uint64), ("records", ctypes.c_uint64), ("slot_words", ctypes.c_uint64),
                ("slots", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FlowTrackUpdate(ctypes.Structure):
    """bt_flow_track_update: ts (n u64, optional) or the scalar batch_ts."""
    _fields_ = [("ts", ctypes.c_void_p), ("batch_ts", ctypes.c_uint64)]


class FlowTrackResult(_Counts):
    """bt_flow_track_result (64 B): the counts of an update."""
    _fields_ = [("n", ctypes.c_uint32), ("n_selected", ctypes.c_uint32), ("none_packets", ctypes.c_uint32),
                ("batch_flows", ctypes.c_uint32), ("new_flows", ctypes.c_uint32), ("overflow_flows", ctypes.c_uint32),
                ("overflow_packets", ctypes.c_uint32), ("n_flows", ctypes.c_uint32), ("seq", ctypes.c_uint32),
                ("status", ctypes.c_uint32), ("keyed_bytes", ctypes.c_uint64), ("none_bytes", ctypes.c_uint64),
                ("overflow_bytes", ctypes.c_uint64)]


class FlowTrackOut(ctypes.Structure):
    _fields_ = [("flow_id", ctypes.c_void_p), ("result", ctypes.c_void_p)]


class FlowTrackExpireResult(_Counts):
    """bt_flow_track_expire_result (32 B)."""
    _fields_ = [("n_flows_before", ctypes.c_uint32), ("n_flows", ctypes.c_uint32), ("n_idle", ctypes.c_uint32),
                ("n_expired", ctypes.c_uint32), ("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class FlowTrackExpireOut(ctypes.Structure):
    _fields_ = [("expired", ctypes.c_void_p), ("expired_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("remap", ctypes.c_void_p), ("result", ctypes.c_void_p)]


def flow_track_layout(flow_cap: int, slots: int = 0) -> dict:
    """bt_flow_track_layout (host only): total bytes, the offsets of header, records and slot words, the resolved slots."""
    s = FlowTrackSizes()
    _check(lib().bt_flow_track_layout(flow_cap, slots, ctypes.byref(s)))
    return s.as_dict()


def flow_track_scratch_bytes(n: int) -> int:
    """bt_flow_track_scratch_bytes (host only): the scratch an update of n packets needs."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_track_scratch_bytes(n, ctypes.byref(b)))
    return b.value


def flow_track_expire_scratch_bytes(flow_cap: int) -> int:
    """bt_flow_track_expire_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_track_expire_scratch_bytes(flow_cap, ctypes.byref(b)))
    return b.value


def flow_track_parse(state, flow_cap: int | None = None) -> tuple:
    """(header dict, records [n_flows] FlowTrackRec) of a tracker state's bytes (at least header and records)."""
    a = _byte_view(state)
    hdr = FlowTrackHdr.from_bytes(a).as_dict()
    lay = flow_track_layout(hdr["flow_cap"], hdr["slots"])
    recs = a[lay["records"]:lay["records"] + 104 * hdr["n_flows"]].copy().view(FlowTrackRec)
    return hdr, recs


class HostFlowTracker:
    """A tracker state in host memory (bt_flow_track_init_host / _update_host / _expire_host)."""

    def __init__(self, flow_cap: int, flags: int = 0, slots: int = 0):
        self.layout = flow_track_layout(flow_cap, slots)
        self.flow_cap = flow_cap
        raw = np.zeros(self.layout["total"] + 256, np.uint8)
        at = -raw.ctypes.data % 256
        self.state = raw[at:at + self.layout["total"]]
        opts = FlowTrackOpts(flags, flow_cap, slots, 0)
        _check(lib().bt_flow_track_init_host(self.state.ctypes.data, self.state.nbytes, ctypes.byref(opts)))

    def update(self, data, desc, select=None, ts=None, batch_ts: int = 0, nbytes=None) -> tuple:
        """One batch (packed descriptors into data). Returns (flow_id [n] u32, result dict)."""
        a = _byte_view(data)
        keep = a if len(a) else np.zeros(1, np.uint8)
        d = np.ascontiguousarray(desc, np.uint64)
        n = len(d)
        sel = None if select is None else np.ascontiguousarray(select, np.uint64)
        t = None if ts is None else np.ascontiguousarray(ts, np.uint64)
        flow_id = np.zeros(max(1, n), np.uint32)
        res = FlowTrackResult()
        upd = FlowTrackUpdate(t.ctypes.data if t is not None and len(t) else None, batch_ts)
        _check(lib().bt_flow_track_update_host(self.state.ctypes.data, self.state.nbytes, keep.ctypes.data,
                                               len(a) if nbytes is None else nbytes, d.ctypes.data if n else None, n,
                                               sel.ctypes.data if sel is not None and len(sel) else None, ctypes.byref(upd),
                                               flow_id.ctypes.data, ctypes.byref(res)))
        return flow_id[:n], res.as_dict()

    def expire(self, now: int, idle: int, expired_cap: int | None = None, want_remap: bool = True) -> tuple:
        """Returns (expired records or None when expired_cap is None, remap [flow_cap] u32 or None, result dict)."""
        exp = None if expired_cap is None else np.zeros(max(1, expired_cap), FlowTrackRec)
        remap = np.full(self.flow_cap, 0xEEEEEEEE, np.uint32) if want_remap else None
        res = FlowTrackExpireResult()
        out = FlowTrackExpireOut(exp.ctypes.data if exp is not None else None, expired_cap or 0, 0,
                                 remap.ctypes.data if remap is not None else None, ctypes.addressof(res))
        _check(lib().bt_flow_track_expire_host(self.state.ctypes.data, self.state.nbytes, now, idle, ctypes.byref(out)))
        r = res.as_dict()
        return (None if exp is None else exp[:r["n_expired"]]), remap, r

    def header(self) -> dict:
        return FlowTrackHdr.from_bytes(self.state).as_dict()

    def records(self) -> np.ndarray:
        return flow_track_parse(self.state)[1]

    def tcp_table(self) -> np.ndarray:
        """The tracker's TCP side table (flow_cap FlowTcpRec, zero), made on first use."""
        if getattr(self, "tcp", None) is None:
            self.tcp = np.zeros(self.flow_cap, FlowTcpRec)
        return self.tcp

    def tcp_update(self, data, desc, flow_id, nbytes=None) -> dict:
        """bt_flow_tcp_update_host over the batch update() numbered (flow_id: what it returned), under the
        state's flags, into tcp_table(). Returns the result dict."""
        return flow_tcp_update_host(data, desc, flow_id, self.header()["flags"], self.tcp_table(), nbytes)

    def top(self, metric: int, k: int) -> tuple:
        """bt_flow_track_top_host: the k largest flows by a FLOW_TOP_* metric, with the side table once
        tcp_table() has made it (the TCP metrics need it). Returns (ids, values, records, side records
        or None, result dict)."""
        return flow_track_top_host(self.state, metric, k, getattr(self, "tcp", None))

    def hosts(self, host_cap: int | None = None, slots: int = 0, want_endpoints: bool = True) -> tuple:
        """bt_flow_track_hosts_host: the tracker's flows aggregated per address, with the side table once
        tcp_table() has made it. Returns (host records [n_written] FlowHostRec, endpoint_host
        [2 n_flows] u32 or None, result dict)."""
        return flow_track_hosts_host(self.state, host_cap, slots, getattr(self, "tcp", None), want_endpoints)

    def expire_tcp(self, now: int, idle: int, closed_idle: int, expired_cap: int | None = None, want_remap: bool = True) -> tuple:
        """bt_flow_track_expire_tcp_host with tcp_table(). Returns (expired records or None, their side
        records or None, remap [flow_cap] u32 or None, result dict)."""
        exp = None if expired_cap is None else np.zeros(max(1, expired_cap), FlowTrackRec)
        exp_tcp = None if expired_cap is None else np.zeros(max(1, expired_cap), FlowTcpRec)
        remap = np.full(self.flow_cap, 0xEEEEEEEE, np.uint32) if want_remap else None
        res = FlowTrackExpireResult()
        out = FlowTrackExpireOut(exp.ctypes.data if exp is not None else None, expired_cap or 0, 0,
                                 remap.ctypes.data if remap is not None else None, ctypes.addressof(res))
        x = FlowTrackExpireTcp(self.tcp_table().ctypes.data, exp_tcp.ctypes.data if exp_tcp is not None else None, closed_idle)
        _check(lib().bt_flow_track_expire_tcp_host(self.state.ctypes.data, self.state.nbytes, now, idle, ctypes.byref(x),
                                                   ctypes.byref(out)))
        r = res.as_dict()
        ne = r["n_expired"]
        return (None if exp is None else exp[:ne]), (None if exp_tcp is None else exp_tcp[:ne]), remap, r


# TCP flag bits (byte 13 of the TCP header) and the states bt_flow_tcp_state gives
TCPF_FIN, TCPF_SYN, TCPF_RST, TCPF_PSH, TCPF_ACK = 0x01, 0x02, 0x04, 0x08, 0x10
TCP_NONE, TCP_OPENING, TCP_ESTABLISHED, TCP_CLOSING, TCP_CLOSED, TCP_RESET, TCP_MIDSTREAM = range(7)
TCP_STATE_NAMES = ("none", "opening", "established", "closing", "closed", "reset", "midstream")

# numpy view of bt_flow_tcp_rec (16 B): record f of a side table belongs to flow number f
FlowTcpRec = np.dtype({
    "names": ["flags", "pad", "syn_packets", "fin_packets", "rst_packets"],
    "formats": [("u1", 2), ("u1", 2), "<u4", "<u4", "<u4"],
    "offsets": [0, 2, 4, 8, 12],
    "itemsize": 16,
})


class FlowTcpResult(_Counts):
    """bt_flow_tcp_result (32 B): the counts of a side table update."""
    _fields_ = [("n", ctypes.c_uint32), ("tcp_packets", ctypes.c_uint32), ("syn_packets", ctypes.c_uint32),
                ("fin_packets", ctypes.c_uint32), ("rst_packets", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


class FlowTrackExpireTcp(ctypes.Structure):
    """bt_flow_track_expire_tcp (24 B): the side table, where expired side records go, closed_idle."""
    _fields_ = [("tcp", ctypes.c_void_p), ("expired_tcp", ctypes.c_void_p), ("closed_idle", ctypes.c_uint64)]


def flow_tcp_state(flags_fwd: int, flags_rev: int, table_flags: int = 0) -> int:
    """bt_flow_tcp_state (host only, pure): a TCP_* state from the two flag unions; not a sequence-checked machine."""
    return lib().bt_flow_tcp_state(flags_fwd, flags_rev, table_flags)


def flow_tcp_update_host(data, desc, flow_id, table_flags: int, tcp: np.ndarray, nbytes=None) -> dict:
    """bt_flow_tcp_update_host (host only): the frames desc (packed descriptors) lists in `data`, numbered
    by flow_id, added to the side table `tcp` (FlowTcpRec, in place). Returns the result dict."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    ids = np.ascontiguousarray(flow_id, np.uint32)
    if len(ids) != n or tcp.dtype != FlowTcpRec or not tcp.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_tcp_update_host: one flow_id per descriptor and a contiguous FlowTcpRec table")
    res = FlowTcpResult()
    _check(lib().bt_flow_tcp_update_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, d.ctypes.data if n else None, n,
                                         ids.ctypes.data if n else None, table_flags, tcp.ctypes.data if len(tcp) else None,
                                         len(tcp), ctypes.addressof(res)))
    return res.as_dict()


def flow_track_expire_tcp_scratch_bytes(flow_cap: int) -> int:
    """bt_flow_track_expire_tcp_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_track_expire_tcp_scratch_bytes(flow_cap, ctypes.byref(b)))
    return b.value


# bt_flow_stat_rec's seen bits (shifted left by 16 for direction 1)
FSEEN_TCP, FSEEN_UDP, FSEEN_ICMP, FSEEN_ICMP6, FSEEN_OTHER = 0x01, 0x02, 0x04, 0x08, 0x10
FSEEN_FRAGMENT, FSEEN_IP_OPTIONS, FSEEN_VLAN, FSEEN_L4 = 0x20, 0x40, 0x80, 0x100
FSEEN_NAMES = ((FSEEN_TCP, "tcp"), (FSEEN_UDP, "udp"), (FSEEN_ICMP, "icmp"), (FSEEN_ICMP6, "icmp6"), (FSEEN_OTHER, "other"))

# numpy view of bt_flow_stat_rec (128 B): record f of a side table belongs to flow number f
FlowStatRec = np.dtype({
    "names": ["seen", "proto_max", "payload_packets", "ttl_max", "ttl_min_c", "len_max", "len_min_c", "payload_bytes", "len_sq",
              "syn_ts_c", "synack_ts_c", "ack_ts_c"],
    "formats": ["<u4", "<u4", ("<u4", 2), ("<u4", 2), ("<u4", 2), ("<u4", 2), ("<u4", 2), ("<u8", 2), ("<u8", 2), ("<u8", 2),
                ("<u8", 2), ("<u8", 2)],
    "offsets": [0, 4, 8, 16, 24, 32, 40, 48, 64, 80, 96, 112],
    "itemsize": 128,
})


class FlowStatResult(_Counts):
    """bt_flow_stat_result (32 B): the counts of a statistics side table update."""
    _fields_ = [("n", ctypes.c_uint32), ("ip_packets", ctypes.c_uint32), ("l4_packets", ctypes.c_uint32),
                ("tcp_packets", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class FlowStatRttOut(_Counts):
    """bt_flow_stat_rtt_out (32 B)."""
    _fields_ = [("has_initiator", ctypes.c_uint32), ("initiator", ctypes.c_uint32), ("server_valid", ctypes.c_uint32),
                ("client_valid", ctypes.c_uint32), ("rtt_server", ctypes.c_uint64), ("rtt_client", ctypes.c_uint64)]


class FlowSideMove(ctypes.Structure):
    """bt_flow_side_move (48 B): a side table, where expired side records go, the expire's remap and result."""
    _fields_ = [("side", ctypes.c_void_p), ("expired_side", ctypes.c_void_p), ("remap", ctypes.c_void_p), ("result", ctypes.c_void_p),
                ("rec_bytes", ctypes.c_uint32), ("flow_cap", ctypes.c_uint32), ("expired_cap", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


def flow_stat_update_host(data, desc, flow_id, table_flags: int, stat: np.ndarray, ts=None, batch_ts: int = 0, nbytes=None) -> dict:
    """bt_flow_stat_update_host (host only): the frames desc (packed descriptors) lists in `data`, numbered
    by flow_id and stamped ts[i] (or batch_ts), added to the side table `stat` (FlowStatRec, in place).
    Returns the result dict."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    ids = np.ascontiguousarray(flow_id, np.uint32)
    t = None if ts is None else np.ascontiguousarray(ts, np.uint64)
    if len(ids) != n or stat.dtype != FlowStatRec or not stat.flags["C_CONTIGUOUS"] or (t is not None and len(t) != n):
        raise ValueError("flow_stat_update_host: one flow_id (and ts) per descriptor and a contiguous FlowStatRec table")
    res = FlowStatResult()
    upd = FlowTrackUpdate(t.ctypes.data if t is not None and n else None, batch_ts)
    _check(lib().bt_flow_stat_update_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, d.ctypes.data if n else None, n,
                                          ids.ctypes.data if n else None, table_flags, ctypes.byref(upd),
                                          stat.ctypes.data if len(stat) else None, len(stat), ctypes.addressof(res)))
    return res.as_dict()


def flow_stat_rtt(rec) -> dict:
    """bt_flow_stat_rtt (host only, pure): the initiator and the two handshake round-trip times of one
    FlowStatRec, as the dict of bt_flow_stat_rtt_out."""
    r = np.ascontiguousarray(rec, FlowStatRec).reshape(1)
    out = FlowStatRttOut()
    _check(lib().bt_flow_stat_rtt(r.ctypes.data, ctypes.addressof(out)))
    return out.as_dict()


def decode_flow_stat(rec) -> dict:
    """One FlowStatRec in plain values: the complemented minima and stamps undone, None where nothing
    was seen. Lists are per direction."""
    r = np.ascontiguousarray(rec, FlowStatRec).reshape(1)[0]
    inv32 = lambda v: None if int(v) == 0 else 0xFFFFFFFF - int(v)  # noqa: E731
    inv64 = lambda v: None if int(v) == 0 else 0xFFFFFFFFFFFFFFFF - int(v)  # noqa: E731
    seen = int(r["seen"])
    return {
        "seen": [seen & 0xFFFF, seen >> 16],
        "protocols": [name for bit, name in FSEEN_NAMES if (seen | seen >> 16) & bit],
        "proto_max": int(r["proto_max"]),
        "payload_packets": [int(v) for v in r["payload_packets"]],
        "payload_bytes": [int(v) for v in r["payload_bytes"]],
        "ttl_max": [int(v) if int(c) else None for v, c in zip(r["ttl_max"], r["ttl_min_c"])],
        "ttl_min": [inv32(v) for v in r["ttl_min_c"]],
        "len_max": [int(v) if int(c) else None for v, c in zip(r["len_max"], r["len_min_c"])],
        "len_min": [inv32(v) for v in r["len_min_c"]],
        "len_sq": [int(v) for v in r["len_sq"]],
        "syn_ts": [inv64(v) for v in r["syn_ts_c"]],
        "synack_ts": [inv64(v) for v in r["synack_ts_c"]],
        "ack_ts": [inv64(v) for v in r["ack_ts_c"]],
    }


def flow_track_side_move_scratch_bytes(flow_cap: int, rec_bytes: int) -> int:
    """bt_flow_track_side_move_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_track_side_move_scratch_bytes(flow_cap, rec_bytes, ctypes.byref(b)))
    return b.value


def flow_track_side_move_host(side: np.ndarray, remap, result: dict, expired_cap: int | None = None):
    """bt_flow_track_side_move_host: the side table `side` (a contiguous array of flow_cap records, in
    place) through the expire that gave remap (flow_cap u32) and result (its dict). Returns the
    side records of the expired flows ([min(n_expired, expired_cap)]), or None when expired_cap is None."""
    if not side.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_track_side_move_host: a contiguous side table")
    rm = np.ascontiguousarray(remap, np.uint32)
    res = FlowTrackExpireResult(result["n_flows_before"], result["n_flows"], result["n_idle"], result["n_expired"], result["status"],
                                (ctypes.c_uint32 * 3)(0, 0, 0))
    gone = None if expired_cap is None else np.zeros(max(1, expired_cap), side.dtype)
    m = FlowSideMove(side.ctypes.data if len(side) else None, gone.ctypes.data if gone is not None else None,
                     rm.ctypes.data if len(rm) else None, ctypes.addressof(res), side.dtype.itemsize, len(side), expired_cap or 0, 0)
    _check(lib().bt_flow_track_side_move_host(ctypes.byref(m)))
    return None if gone is None else gone[:min(result["n_expired"], expired_cap)]


# bt_flow_mark_select_*: the flag and the ops that combine the marked packets with a base selection
FLOW_MARK_ALL_BITS = 0x1
FLOW_MARK_SET, FLOW_MARK_AND, FLOW_MARK_OR, FLOW_MARK_ANDNOT = range(4)

# numpy view of bt_flow_mark_rec (32 B): record f of a mark table belongs to flow number f
FlowMarkRec = np.dtype({
    "names": ["marks", "hit_packets", "hit_bytes", "first_hit_ts_c", "last_hit_ts"],
    "formats": ["<u4", "<u4", "<u8", "<u8", "<u8"],
    "offsets": [0, 4, 8, 16, 24],
    "itemsize": 32,
})


class FlowMarkUpdate(ctypes.Structure):
    """bt_flow_mark_update (24 B): the mark bits, per-packet timestamps or one for the batch."""
    _fields_ = [("mark", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("ts", ctypes.c_void_p), ("batch_ts", ctypes.c_uint64)]


class FlowMarkResult(_Counts):
    """bt_flow_mark_result (32 B): the counts of a mark table update."""
    _fields_ = [("n", ctypes.c_uint32), ("hit_packets", ctypes.c_uint32), ("marked_packets", ctypes.c_uint32),
                ("unkeyed_hits", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32), ("new_marked_flows", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


class FlowMarkSelectOpts(ctypes.Structure):
    """bt_flow_mark_select_opts (16 B)."""
    _fields_ = [("mask", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("op", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FlowMarkSelectResult(_Counts):
    """bt_flow_mark_select_result (32 B): the counts of a selection by marks."""
    _fields_ = [("n", ctypes.c_uint32), ("n_marked", ctypes.c_uint32), ("n_out", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


def flow_mark_update_host(desc, flow_id, hit, mark: int, table: np.ndarray, ts=None, batch_ts: int = 0) -> dict:
    """bt_flow_mark_update_host (host only): the packets desc (packed descriptors) lists whose bit is
    set in `hit` (verdict-layout u64 words, None = all) raise `mark` on the record of their flow
    number flow_id[i] in `table` (FlowMarkRec, in place), stamped ts[i] (or batch_ts). Returns the
    result dict."""
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    ids = np.ascontiguousarray(flow_id, np.uint32)
    h = None if hit is None else np.ascontiguousarray(hit, np.uint64)
    t = None if ts is None else np.ascontiguousarray(ts, np.uint64)
    if (len(ids) != n or table.dtype != FlowMarkRec or not table.flags["C_CONTIGUOUS"] or (t is not None and len(t) != n)
            or (h is not None and len(h) < (n + 63) // 64)):
        raise ValueError("flow_mark_update_host: one flow_id (and ts) per descriptor, ceil(n/64) hit words and a contiguous "
                         "FlowMarkRec table")
    res = FlowMarkResult()
    upd = FlowMarkUpdate(mark, 0, t.ctypes.data if t is not None and n else None, batch_ts)
    _check(lib().bt_flow_mark_update_host(d.ctypes.data if n else None, n, ids.ctypes.data if n else None,
                                          h.ctypes.data if h is not None and len(h) else None, ctypes.byref(upd),
                                          table.ctypes.data if len(table) else None, len(table), ctypes.addressof(res)))
    return res.as_dict()


def flow_mark_select_host(flow_id, table: np.ndarray, mask: int, op: int = FLOW_MARK_SET, flags: int = 0, base=None, out=None) -> tuple:
    """bt_flow_mark_select_host (host only): the verdict-layout selection of the packets whose flow
    number flow_id[i] carries a bit of `mask` (with FLOW_MARK_ALL_BITS: every bit) in `table`
    (FlowMarkRec), combined with `base` by a FLOW_MARK_* op. out: ceil(n/64) u64 words to write (may
    be base itself), made when None. Returns (out, result dict)."""
    ids = np.ascontiguousarray(flow_id, np.uint32)
    n = len(ids)
    nw = (n + 63) // 64
    if out is None:
        out = np.zeros(nw, np.uint64)
    if (table.dtype != FlowMarkRec or not table.flags["C_CONTIGUOUS"] or out.dtype != np.uint64 or len(out) < nw
            or not out.flags["C_CONTIGUOUS"] or (base is not None and (base.dtype != np.uint64 or len(base) < nw
                                                                         or not base.flags["C_CONTIGUOUS"]))):
        raise ValueError("flow_mark_select_host: a contiguous FlowMarkRec table and ceil(n/64) contiguous u64 words for base and out")
    res = FlowMarkSelectResult()
    opts = FlowMarkSelectOpts(mask, flags, op, 0)
    _check(lib().bt_flow_mark_select_host(ids.ctypes.data if n else None, n, table.ctypes.data if len(table) else None, len(table),
                                          ctypes.byref(opts), base.ctypes.data if base is not None and len(base) else None,
                                          out.ctypes.data if len(out) else None, ctypes.addressof(res)))
    return out, res.as_dict()


def decode_flow_mark(rec) -> dict:
    """One FlowMarkRec in plain values: the complemented first stamp undone, None where the flow was never hit."""
    r = np.ascontiguousarray(rec, FlowMarkRec).reshape(1)[0]
    return {"marks": int(r["marks"]), "hit_packets": int(r["hit_packets"]), "hit_bytes": int(r["hit_bytes"]),
            "first_hit_ts": None if int(r["first_hit_ts_c"]) == 0 else 0xFFFFFFFFFFFFFFFF - int(r["first_hit_ts_c"]),
            "last_hit_ts": int(r["last_hit_ts"]) if int(r["hit_packets"]) else None}


# bt_flow_seq_*: the flag, and what seq / byte_off hold for a packet that was not numbered
FLOW_SEQ_KEEP_UNKEYED = 0x1
FLOW_SEQ_NONE = 0xFFFFFFFF
FLOW_SEQ_MAX = 0xFFFFFFFE
FLOW_SEQ_OFF_NONE = 0xFFFFFFFFFFFFFFFF

# numpy view of bt_flow_seq_rec (16 B): record f of a sequence table belongs to flow number f
FlowSeqRec = np.dtype({"names": ["packets", "bytes"], "formats": ["<u8", "<u8"], "offsets": [0, 8], "itemsize": 16})


class FlowSeqOpts(ctypes.Structure):
    """bt_flow_seq_opts (32 B): the per-flow limits (0 = none) and FLOW_SEQ_* flags."""
    _fields_ = [("max_packets", ctypes.c_uint64), ("max_bytes", ctypes.c_uint64), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 3)]


class FlowSeqOut(ctypes.Structure):
    """bt_flow_seq_out (24 B): the three optional outputs."""
    _fields_ = [("seq", ctypes.c_void_p), ("byte_off", ctypes.c_void_p), ("out_select", ctypes.c_void_p)]


class FlowSeqResult(_Counts):
    """bt_flow_seq_result (64 B): the counts of a numbering call."""
    _fields_ = [("n", ctypes.c_uint32), ("selected", ctypes.c_uint32), ("numbered", ctypes.c_uint32), ("unkeyed", ctypes.c_uint32),
                ("bad_ids", ctypes.c_uint32), ("kept", ctypes.c_uint32), ("flows", ctypes.c_uint32), ("new_flows", ctypes.c_uint32),
                ("numbered_bytes", ctypes.c_uint64), ("kept_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 2)]


def flow_seq_scratch_bytes(n: int, flow_cap: int) -> int:
    """bt_flow_seq_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_seq_scratch_bytes(n, flow_cap, ctypes.byref(b)))
    return b.value


def flow_seq_host(desc, flow_id, select, table: np.ndarray, max_packets: int = 0, max_bytes: int = 0, flags: int = 0,
                  seq=None, byte_off=None, out_select=None) -> dict:
    """bt_flow_seq_host (host only): the packets desc (packed descriptors) lists whose bit is set in
    `select` (verdict-layout u64 words, None = all) and whose flow number flow_id[i] is below
    len(table) are numbered inside their flow against `table` (FlowSeqRec, in place). seq (n u32),
    byte_off (n u64) and out_select (ceil(n/64) u64 words, may be `select`) are written where given.
    Returns the result dict."""
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    nw = (n + 63) // 64
    ids = np.ascontiguousarray(flow_id, np.uint32)
    sel = select
    if sel is not None and (sel.dtype != np.uint64 or not sel.flags["C_CONTIGUOUS"] or len(sel) < nw):
        raise ValueError("flow_seq_host: ceil(n/64) contiguous u64 select words")
    for arr, dt, need in ((seq, np.uint32, n), (byte_off, np.uint64, n), (out_select, np.uint64, nw)):
        if arr is not None and (arr.dtype != dt or not arr.flags["C_CONTIGUOUS"] or len(arr) < need):
            raise ValueError("flow_seq_host: contiguous outputs of n u32, n u64 and ceil(n/64) u64")
    if len(ids) != n or table.dtype != FlowSeqRec or not table.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_seq_host: one flow_id per descriptor and a contiguous FlowSeqRec table")
    at = lambda x: x.ctypes.data if x is not None and len(x) else None  # noqa: E731
    res = FlowSeqResult()
    opts = FlowSeqOpts(max_packets, max_bytes, flags, (ctypes.c_uint32 * 3)(0, 0, 0))
    out = FlowSeqOut(at(seq), at(byte_off), at(out_select))
    _check(lib().bt_flow_seq_host(at(d), n, at(ids), at(sel), ctypes.byref(opts), at(table), len(table), ctypes.byref(out),
                                  ctypes.addressof(res)))
    return res.as_dict()


def decode_flow_seq(seq, byte_off) -> list:
    """seq and byte_off of a numbering call in plain values: (packets before, bytes before) per
    packet, None for a packet that was not numbered; a seq of FLOW_SEQ_MAX means "at least"."""
    s = np.asarray(seq, np.uint32)
    b = np.asarray(byte_off, np.uint64)
    return [None if int(x) == FLOW_SEQ_NONE else (int(x), int(y)) for x, y in zip(s, b)]


# numpy view of bt_flow_stream_rec (32 B): record f of a stream table belongs to flow number f
FlowStreamRec = np.dtype({"names": ["d", "hit_packets", "stream_packets"], "formats": [("<u8", 2), ("<u4", 2), ("<u4", 2)],
                          "offsets": [0, 16, 24], "itemsize": 32})


class FlowStreamInfo(_Counts):
    """bt_flow_stream_info (16 B): the blob's entry width W, the pattern's positions P, the tail T = P - 1 and the closure steps R."""
    _fields_ = [("width", ctypes.c_uint32), ("positions", ctypes.c_uint32), ("tail", ctypes.c_uint32), ("closure", ctypes.c_uint32)]


class FlowStreamOut(ctypes.Structure):
    """bt_flow_stream_out (32 B): the optional hit words and the result."""
    _fields_ = [("hit", ctypes.c_void_p), ("result", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2)]


class FlowStreamResult(_Counts):
    """bt_flow_stream_result (64 B): the counts of a stream matching call."""
    _fields_ = [("n", ctypes.c_uint32), ("selected", ctypes.c_uint32), ("stream_packets", ctypes.c_uint32),
                ("hit_packets", ctypes.c_uint32), ("unkeyed", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32),
                ("stream_bytes", ctypes.c_uint64), ("new_hit_flows", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


def flow_stream_compile(expression: str):
    """bt_flow_stream_compile (host only): (blob as a u8 array, info dict) of a pattern the stream
    matcher takes. BtError BT_E_NOT_IMPLEMENTED names the construct it refuses (+, *, {n,}, ^, $, \\b,
    a pattern only the DFA takes, the always / never forms); BT_E_INVALID_ARGUMENT: not a regex."""
    e = expression.encode()
    size = ctypes.c_uint32(0)
    info = FlowStreamInfo()
    _check(lib().bt_flow_stream_compile(e, None, 0, ctypes.byref(size), ctypes.addressof(info)))
    blob = np.zeros(size.value, np.uint8)
    _check(lib().bt_flow_stream_compile(e, blob.ctypes.data, size.value, ctypes.byref(size), ctypes.addressof(info)))
    return blob, info.as_dict()


def flow_stream_scratch_bytes(n: int, flow_cap: int) -> int:
    """bt_flow_stream_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_stream_scratch_bytes(n, flow_cap, ctypes.byref(b)))
    return b.value


def flow_stream_host(data, desc, flow_id, select, table_flags: int, pattern, table: np.ndarray, hit=None, nbytes=None) -> dict:
    """bt_flow_stream_host (host only): the L4 payloads of the frames desc (packed descriptors) lists
    in `data` whose bit is set in `select` (verdict-layout u64 words, None = all) and whose flow
    number flow_id[i] is below len(table) are appended to their (flow, direction) streams, and
    `pattern` (flow_stream_compile's blob) is matched across them against `table` (FlowStreamRec, in
    place). hit (ceil(n/64) u64 words, may be `select`) gets the packets in which a match ends.
    Returns the result dict."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    nw = (n + 63) // 64
    ids = np.ascontiguousarray(flow_id, np.uint32)
    pat = np.ascontiguousarray(pattern, np.uint8)
    for arr in (select, hit):
        if arr is not None and (arr.dtype != np.uint64 or not arr.flags["C_CONTIGUOUS"] or len(arr) < nw):
            raise ValueError("flow_stream_host: ceil(n/64) contiguous u64 words for select and hit")
    if len(ids) != n or table.dtype != FlowStreamRec or not table.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_stream_host: one flow_id per descriptor and a contiguous FlowStreamRec table")
    at = lambda x: x.ctypes.data if x is not None and len(x) else None  # noqa: E731
    res = FlowStreamResult()
    out = FlowStreamOut(at(hit), ctypes.addressof(res), (ctypes.c_uint64 * 2)(0, 0))
    _check(lib().bt_flow_stream_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, at(d), n, at(ids), at(select),
                                     table_flags, at(pat), len(pat), at(table), len(table), ctypes.byref(out)))
    return res.as_dict()


def decode_flow_stream(rec) -> dict:
    """One FlowStreamRec in plain values, per direction: the matcher's state, the packets of the
    stream and those in which a match ended."""
    r = np.ascontiguousarray(rec, FlowStreamRec).reshape(1)[0]
    return {"state": [int(r["d"][0]), int(r["d"][1])], "stream_packets": [int(r["stream_packets"][0]), int(r["stream_packets"][1])],
            "hit_packets": [int(r["hit_packets"][0]), int(r["hit_packets"][1])],
            "hit": bool(int(r["hit_packets"][0]) or int(r["hit_packets"][1]))}


# bt_flow_tcpseq_*: a segment's class against its direction's sequence space, and "not classified" in off
TCPSEQ_NONE, TCPSEQ_FIRST, TCPSEQ_IN_ORDER, TCPSEQ_GAP, TCPSEQ_OLD, TCPSEQ_OVERLAP = range(6)
TCPSEQ_NAMES = ("none", "first", "in_order", "gap", "old", "overlap")
TCPSEQ_OFF_NONE = -(1 << 63)

# numpy views of bt_flow_tcpseq_dir (64 B) and bt_flow_tcpseq_rec (128 B, one per direction): record f belongs to flow number f
FlowTcpseqDir = np.dtype({"names": ["pos", "hi", "last_seq", "have", "seq_packets", "old_packets", "gap_packets", "overlap_packets",
                                    "old_bytes", "gap_bytes", "reserved"],
                          "formats": ["<i8", "<i8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8"],
                          "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56], "itemsize": 64})
FlowTcpseqRec = np.dtype({"names": ["d"], "formats": [(FlowTcpseqDir, 2)], "offsets": [0], "itemsize": 128})


class FlowTcpseqOut(ctypes.Structure):
    """bt_flow_tcpseq_out (48 B): the optional class bytes, offsets and selection words, and the result."""
    _fields_ = [("cls", ctypes.c_void_p), ("off", ctypes.c_void_p), ("out_select", ctypes.c_void_p), ("result", ctypes.c_void_p),
                ("reserved", ctypes.c_uint64 * 2)]


class FlowTcpseqResult(_Counts):
    """bt_flow_tcpseq_result (64 B): the counts of a TCP sequence classification call."""
    _fields_ = [("n", ctypes.c_uint32), ("selected", ctypes.c_uint32), ("seq_packets", ctypes.c_uint32), ("first", ctypes.c_uint32),
                ("in_order", ctypes.c_uint32), ("gap", ctypes.c_uint32), ("old", ctypes.c_uint32), ("overlap", ctypes.c_uint32),
                ("unkeyed", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32), ("seq_bytes", ctypes.c_uint64),
                ("old_bytes", ctypes.c_uint64), ("gap_bytes", ctypes.c_uint64)]


def flow_tcpseq_scratch_bytes(n: int, flow_cap: int) -> int:
    """bt_flow_tcpseq_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_tcpseq_scratch_bytes(n, flow_cap, ctypes.byref(b)))
    return b.value


def flow_tcpseq_host(data, desc, flow_id, select, table_flags: int, table: np.ndarray, cls=None, off=None, out_select=None,
                     nbytes=None) -> dict:
    """bt_flow_tcpseq_host (host only): the TCP segments of the frames desc (packed descriptors) lists
    in `data` whose bit is set in `select` (verdict-layout u64 words, None = all) and whose flow
    number flow_id[i] is below len(table) are placed in their (flow, direction) sequence space and
    classified against `table` (FlowTcpseqRec, in place). cls (n u8), off (n i8) and out_select
    (ceil(n/64) u64 words, may be `select`: select & ~OLD) are optional. Returns the result dict."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    nw = (n + 63) // 64
    ids = np.ascontiguousarray(flow_id, np.uint32)
    for arr in (select, out_select):
        if arr is not None and (arr.dtype != np.uint64 or not arr.flags["C_CONTIGUOUS"] or len(arr) < nw):
            raise ValueError("flow_tcpseq_host: ceil(n/64) contiguous u64 words for select and out_select")
    if cls is not None and (cls.dtype != np.uint8 or not cls.flags["C_CONTIGUOUS"] or len(cls) < n):
        raise ValueError("flow_tcpseq_host: n contiguous u8 for cls")
    if off is not None and (off.dtype != np.int64 or not off.flags["C_CONTIGUOUS"] or len(off) < n):
        raise ValueError("flow_tcpseq_host: n contiguous i8 for off")
    if len(ids) != n or table.dtype != FlowTcpseqRec or not table.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_tcpseq_host: one flow_id per descriptor and a contiguous FlowTcpseqRec table")
    at = lambda x: x.ctypes.data if x is not None and len(x) else None  # noqa: E731
    res = FlowTcpseqResult()
    out = FlowTcpseqOut(at(cls), at(off), at(out_select), ctypes.addressof(res), (ctypes.c_uint64 * 2)(0, 0))
    _check(lib().bt_flow_tcpseq_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, at(d), n, at(ids), at(select),
                                     table_flags, at(table), len(table), ctypes.byref(out)))
    return res.as_dict()


def decode_flow_tcpseq(rec) -> dict:
    """One FlowTcpseqRec in plain values, per direction: whether the direction was seen, its last
    packet's offset and sequence number, the highest offset seen, and the packets and bytes that
    were old (retransmitted or late), ahead of a gap or overlapping."""
    r = np.ascontiguousarray(rec, FlowTcpseqRec).reshape(1)[0]
    names = ("seq_packets", "old_packets", "gap_packets", "overlap_packets", "old_bytes", "gap_bytes")
    out = {"have": [bool(int(r["d"][k]["have"])) for k in range(2)], "pos": [int(r["d"][k]["pos"]) for k in range(2)],
           "hi": [int(r["d"][k]["hi"]) for k in range(2)], "last_seq": [int(r["d"][k]["last_seq"]) for k in range(2)]}
    for name in names:
        out[name] = [int(r["d"][k][name]) for k in range(2)]
    return out


# numpy views of bt_flow_reasm_dir (64 B) and bt_flow_reasm_rec (128 B, one per direction): record f belongs to flow number f
FlowReasmDir = np.dtype({"names": ["d", "next", "have", "stream_packets", "hit_packets", "holes", "dup_packets", "late_packets",
                                   "dup_bytes", "hole_bytes", "late_bytes"],
                         "formats": ["<u8", "<i8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8"],
                         "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56], "itemsize": 64})
FlowReasmRec = np.dtype({"names": ["d"], "formats": [(FlowReasmDir, 2)], "offsets": [0], "itemsize": 128})


class FlowReasmOut(ctypes.Structure):
    """bt_flow_reasm_out (40 B): the optional hit and rest words, and the result."""
    _fields_ = [("hit", ctypes.c_void_p), ("rest", ctypes.c_void_p), ("result", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2)]


class FlowReasmResult(_Counts):
    """bt_flow_reasm_result (64 B): the counts of a reassembly call."""
    _fields_ = [("n", ctypes.c_uint32), ("selected", ctypes.c_uint32), ("unkeyed", ctypes.c_uint32), ("bad_ids", ctypes.c_uint32),
                ("stream_packets", ctypes.c_uint32), ("hit_packets", ctypes.c_uint32), ("new_hit_flows", ctypes.c_uint32),
                ("holes", ctypes.c_uint32), ("dup_packets", ctypes.c_uint32), ("late_packets", ctypes.c_uint32),
                ("far_packets", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("stream_bytes", ctypes.c_uint64),
                ("reserved1", ctypes.c_uint64)]


def flow_reasm_scratch_bytes(n: int, flow_cap: int) -> int:
    """bt_flow_reasm_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_reasm_scratch_bytes(n, flow_cap, ctypes.byref(b)))
    return b.value


def flow_reasm_host(data, desc, flow_id, select, off, table_flags: int, pattern, table: np.ndarray, hit=None, rest=None,
                    nbytes=None) -> dict:
    """bt_flow_reasm_host (host only): the TCP segments of the frames desc (packed descriptors) lists
    in `data` whose bit is set in `select` (verdict-layout u64 words, None = all), whose flow number
    flow_id[i] is below len(table) and which flow_tcpseq placed (`off`, n int64, its output for the
    same select) are ordered by sequence position per (flow, direction), trimmed where they overlap,
    and `pattern` (flow_stream_compile's blob) is matched over the bytes in that order against
    `table` (FlowReasmRec, in place). hit and rest (ceil(n/64) u64 words each; either may be
    `select`): the packets from whose delivered bytes a match ends, and the selected packets that
    were not placed. Returns the result dict."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    nw = (n + 63) // 64
    ids = np.ascontiguousarray(flow_id, np.uint32)
    pat = np.ascontiguousarray(pattern, np.uint8)
    for arr in (select, hit, rest):
        if arr is not None and (arr.dtype != np.uint64 or not arr.flags["C_CONTIGUOUS"] or len(arr) < nw):
            raise ValueError("flow_reasm_host: ceil(n/64) contiguous u64 words for select, hit and rest")
    if (off is None and n) or (off is not None and (off.dtype != np.int64 or not off.flags["C_CONTIGUOUS"] or len(off) < n)):
        raise ValueError("flow_reasm_host: n contiguous i8 for off")
    if len(ids) != n or table.dtype != FlowReasmRec or not table.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_reasm_host: one flow_id per descriptor and a contiguous FlowReasmRec table")
    at = lambda x: x.ctypes.data if x is not None and len(x) else None  # noqa: E731
    res = FlowReasmResult()
    out = FlowReasmOut(at(hit), at(rest), ctypes.addressof(res), (ctypes.c_uint64 * 2)(0, 0))
    _check(lib().bt_flow_reasm_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, at(d), n, at(ids), at(select), at(off),
                                    table_flags, at(pat), len(pat), at(table), len(table), ctypes.byref(out)))
    return res.as_dict()


def decode_flow_reasm(rec) -> dict:
    """One FlowReasmRec in plain values, per direction: whether the direction was seen, the position
    up to which its stream was delivered, the matcher's state, and its packets, hits, holes,
    duplicates and late segments."""
    r = np.ascontiguousarray(rec, FlowReasmRec).reshape(1)[0]
    names = ("stream_packets", "hit_packets", "holes", "dup_packets", "late_packets", "dup_bytes", "hole_bytes", "late_bytes")
    out = {"have": [bool(int(r["d"][k]["have"])) for k in range(2)], "next": [int(r["d"][k]["next"]) for k in range(2)],
           "state": [int(r["d"][k]["d"]) for k in range(2)]}
    for name in names:
        out[name] = [int(r["d"][k][name]) for k in range(2)]
    out["hit"] = bool(out["hit_packets"][0] or out["hit_packets"][1])
    return out


# bt_flow_follow_*: the flag bits of a run, and bt_flow_follow_run (32 B) as a numpy view
FOLLOW_DIR, FOLLOW_NEW, FOLLOW_HOLE = 1, 2, 4
FlowFollowRun = np.dtype({"names": ["flow", "flags", "at", "pos", "len"], "formats": ["<u4", "<u4", "<u8", "<i8", "<u8"],
                          "offsets": [0, 4, 8, 16, 24], "itemsize": 32})


class FlowFollowOut(ctypes.Structure):
    """bt_flow_follow_out (64 B): the bytes and their capacity, the runs and theirs, the optional place array, the result."""
    _fields_ = [("bytes", ctypes.c_void_p), ("cap", ctypes.c_uint64), ("runs", ctypes.c_void_p), ("run_cap", ctypes.c_uint32),
                ("reserved0", ctypes.c_uint32), ("place", ctypes.c_void_p), ("result", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2)]


class FlowFollowResult(_Counts):
    """bt_flow_follow_result (32 B): the bytes and runs of a follow call, and how many of each were written."""
    _fields_ = [("total", ctypes.c_uint64), ("written", ctypes.c_uint64), ("n_runs", ctypes.c_uint32), ("runs_written", ctypes.c_uint32),
                ("reserved", ctypes.c_uint64)]


def flow_follow_scratch_bytes(n: int, flow_cap: int) -> int:
    """bt_flow_follow_scratch_bytes (host only)."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_follow_scratch_bytes(n, flow_cap, ctypes.byref(b)))
    return b.value


def flow_follow_host(data, desc, flow_id, select, off, table_flags: int, pattern, table: np.ndarray, out_bytes=None, runs=None,
                     place=None, hit=None, rest=None, nbytes=None) -> tuple:
    """bt_flow_follow_host (host only): flow_reasm_host's work on `table` (FlowReasmRec, in place), with
    every delivered byte written to out_bytes (a contiguous u8 array, its length the capacity; None:
    a size query), the runs between holes to runs (a contiguous FlowFollowRun array, its length the
    capacity; None: none) and each packet's output offset to place (n u64; optional). pattern: a
    flow_stream_compile blob, or None for the plain follow (nothing matched, hit zero). Returns (the
    reassembly's result dict, the follow's result dict)."""
    a = _byte_view(data)
    keep = a if len(a) else np.zeros(1, np.uint8)
    d = np.ascontiguousarray(desc, np.uint64)
    n = len(d)
    nw = (n + 63) // 64
    ids = np.ascontiguousarray(flow_id, np.uint32)
    pat = None if pattern is None else np.ascontiguousarray(pattern, np.uint8)
    for arr in (select, hit, rest):
        if arr is not None and (arr.dtype != np.uint64 or not arr.flags["C_CONTIGUOUS"] or len(arr) < nw):
            raise ValueError("flow_follow_host: ceil(n/64) contiguous u64 words for select, hit and rest")
    if (off is None and n) or (off is not None and (off.dtype != np.int64 or not off.flags["C_CONTIGUOUS"] or len(off) < n)):
        raise ValueError("flow_follow_host: n contiguous i8 for off")
    if len(ids) != n or table.dtype != FlowReasmRec or not table.flags["C_CONTIGUOUS"]:
        raise ValueError("flow_follow_host: one flow_id per descriptor and a contiguous FlowReasmRec table")
    if out_bytes is not None and (out_bytes.dtype != np.uint8 or not out_bytes.flags["C_CONTIGUOUS"]):
        raise ValueError("flow_follow_host: a contiguous u8 array for out_bytes")
    if runs is not None and (runs.dtype != FlowFollowRun or not runs.flags["C_CONTIGUOUS"]):
        raise ValueError("flow_follow_host: a contiguous FlowFollowRun array for runs")
    if place is not None and (place.dtype != np.uint64 or not place.flags["C_CONTIGUOUS"] or len(place) < n):
        raise ValueError("flow_follow_host: n contiguous u64 for place")
    at = lambda x: x.ctypes.data if x is not None and len(x) else None  # noqa: E731
    res, fres = FlowReasmResult(), FlowFollowResult()
    out = FlowReasmOut(at(hit), at(rest), ctypes.addressof(res), (ctypes.c_uint64 * 2)(0, 0))
    fo = FlowFollowOut(at(out_bytes), 0 if out_bytes is None else len(out_bytes), at(runs), 0 if runs is None else len(runs), 0,
                       at(place), ctypes.addressof(fres), (ctypes.c_uint64 * 2)(0, 0))
    _check(lib().bt_flow_follow_host(keep.ctypes.data, len(a) if nbytes is None else nbytes, at(d), n, at(ids), at(select), at(off),
                                     table_flags, at(pat), 0 if pat is None else len(pat), at(table), len(table), ctypes.byref(out),
                                     ctypes.byref(fo)))
    return res.as_dict(), fres.as_dict()


# bt_flow_track_top_*: the metric a top-K query orders by, and its limit on k
FLOW_TOP_BYTES, FLOW_TOP_PACKETS, FLOW_TOP_DURATION, FLOW_TOP_TCP_SYN, FLOW_TOP_TCP_RST = range(5)
FLOW_TOP_MAX_K = 4096


class FlowTopOpts(ctypes.Structure):
    """bt_flow_top_opts: a FLOW_TOP_* metric and k <= FLOW_TOP_MAX_K."""
    _fields_ = [("metric", ctypes.c_uint32), ("k", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class FlowTopResult(_Counts):
    """bt_flow_top_result (48 B): what a top-K query found."""
    _fields_ = [("n_flows", ctypes.c_uint32), ("n_top", ctypes.c_uint32), ("status", ctypes.c_uint32), ("metric", ctypes.c_uint32),
                ("n_ties", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("threshold", ctypes.c_uint64),
                ("total", ctypes.c_uint64), ("top_total", ctypes.c_uint64)]


class FlowTopOut(ctypes.Structure):
    """bt_flow_top_out: k entries each, all optional but result."""
    _fields_ = [("top_id", ctypes.c_void_p), ("top_value", ctypes.c_void_p), ("top", ctypes.c_void_p), ("top_tcp", ctypes.c_void_p),
                ("result", ctypes.c_void_p)]


def flow_track_top_scratch_bytes(flow_cap: int, k: int) -> int:
    """bt_flow_track_top_scratch_bytes (host only): the scratch a top-k query over a tracker of flow_cap flows needs."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_track_top_scratch_bytes(flow_cap, k, ctypes.byref(b)))
    return b.value


def flow_track_top_host(state: np.ndarray, metric: int, k: int, tcp: np.ndarray | None = None, want_tcp: bool | None = None) -> tuple:
    """bt_flow_track_top_host (host only) over a tracker state's bytes (256-byte aligned) and, optionally,
    its side table. Returns (ids [n_top] u32, values [n_top] u64, records [n_top] FlowTrackRec, side
    records [n_top] FlowTcpRec or None, result dict)."""
    n = max(1, k)
    ids, vals, recs = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, FlowTrackRec)
    side = np.zeros(n, FlowTcpRec) if (tcp is not None if want_tcp is None else want_tcp) else None
    res = FlowTopResult()
    opts = FlowTopOpts(metric, k, (ctypes.c_uint32 * 2)(0, 0))
    out = FlowTopOut(ids.ctypes.data, vals.ctypes.data, recs.ctypes.data, side.ctypes.data if side is not None else None,
                     ctypes.addressof(res))
    _check(lib().bt_flow_track_top_host(state.ctypes.data, state.nbytes, ctypes.byref(opts), tcp.ctypes.data if tcp is not None else None,
                                        ctypes.byref(out)))
    r = res.as_dict()
    nt = r["n_top"]
    return ids[:nt], vals[:nt], recs[:nt], (None if side is None else side[:nt]), r


FlowHostRec = np.dtype({
    "names": ["addr", "family", "pad", "first_flow", "flows", "packets", "bytes", "first_ts", "last_ts", "tcp_state", "syn_flows",
              "syn_packets", "fin_packets", "rst_packets"],
    "formats": [("u1", 16), "u1", ("u1", 3), "<u4", ("<u4", 2), ("<u8", 2), ("<u8", 2), "<u8", "<u8", ("<u4", 7), ("<u4", 2),
                "<u4", "<u4", "<u4"],
    "offsets": [0, 16, 17, 20, 24, 32, 48, 64, 72, 80, 108, 116, 120, 124],
    "itemsize": 128,
})


class FlowHostsOpts(ctypes.Structure):
    """bt_flow_hosts_opts: the endpoint table's slots (0 = auto, 4 flow_cap) and how many host records to write."""
    _fields_ = [("slots", ctypes.c_uint32), ("host_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class FlowHostsResult(_Counts):
    """bt_flow_hosts_result (64 B): what an endpoint-table query found."""
    _fields_ = [("n_flows", ctypes.c_uint32), ("n_hosts", ctypes.c_uint32), ("n_written", ctypes.c_uint32), ("status", ctypes.c_uint32),
                ("overflow_endpoints", ctypes.c_uint32), ("slots", ctypes.c_uint32), ("hosts_v4", ctypes.c_uint32),
                ("hosts_v6", ctypes.c_uint32), ("packets_total", ctypes.c_uint64), ("bytes_total", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 2)]


class FlowHostsOut(ctypes.Structure):
    """bt_flow_hosts_out: host_cap records, 2 flow_cap host numbers (optional), the result (required)."""
    _fields_ = [("hosts", ctypes.c_void_p), ("endpoint_host", ctypes.c_void_p), ("result", ctypes.c_void_p)]


def flow_track_hosts_scratch_bytes(flow_cap: int, slots: int = 0) -> int:
    """bt_flow_track_hosts_scratch_bytes (host only): the scratch an endpoint-table query over a tracker of flow_cap flows needs."""
    b = ctypes.c_uint64(0)
    _check(lib().bt_flow_track_hosts_scratch_bytes(flow_cap, slots, ctypes.byref(b)))
    return b.value


def flow_track_hosts_host(state: np.ndarray, host_cap: int | None = None, slots: int = 0, tcp: np.ndarray | None = None,
                          want_endpoints: bool = True) -> tuple:
    """bt_flow_track_hosts_host (host only) over a tracker state's bytes (256-byte aligned) and, optionally,
    its side table. host_cap None = room for every host. Returns (host records [n_written] FlowHostRec,
    endpoint_host [2 n_flows] u32 or None, result dict)."""
    hdr = FlowTrackHdr.from_bytes(state[:128]).as_dict()
    cap = 2 * hdr["flow_cap"] if host_cap is None else host_cap
    hosts = np.zeros(max(1, cap), FlowHostRec)
    ends = np.zeros(max(1, 2 * hdr["flow_cap"]), np.uint32) if want_endpoints else None
    res = FlowHostsResult()
    opts = FlowHostsOpts(slots, cap, (ctypes.c_uint32 * 2)(0, 0))
    out = FlowHostsOut(hosts.ctypes.data, ends.ctypes.data if ends is not None else None, ctypes.addressof(res))
    _check(lib().bt_flow_track_hosts_host(state.ctypes.data, state.nbytes, ctypes.byref(opts), tcp.ctypes.data if tcp is not None else None,
                                          ctypes.byref(out)))
    r = res.as_dict()
    return hosts[:r["n_written"]], (None if ends is None else ends[:2 * r["n_flows"]]), r


class PcapInfo(ctypes.Structure):
    """bt_pcap_info: what bt_pcap_index read from a capture file's global header."""
    _fields_ = [("magic", ctypes.c_uint32), ("swapped", ctypes.c_uint32), ("nanosecond", ctypes.c_uint32),
                ("snaplen", ctypes.c_uint32), ("linktype", ctypes.c_uint32), ("truncated", ctypes.c_uint32),
                ("end", ctypes.c_uint64)]


class PcapResult(ctypes.Structure):
    """bt_pcap_result: bt_pcap_filter's counts."""
    _fields_ = [("n_in", ctypes.c_uint64), ("n_pass", ctypes.c_uint64), ("n_reject", ctypes.c_uint64),
                ("n_throw", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("truncated", ctypes.c_uint32),
                ("chunks", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Timing(ctypes.Structure):
    """bt_timing (include/beatrice_gpu.h): bt_time_device_ex's breakdown."""
    _fields_ = [("span_ms", ctypes.c_float), ("main_ms", ctypes.c_float), ("main_min_ms", ctypes.c_float),
                ("main_max_ms", ctypes.c_float), ("lead_ms", ctypes.c_float), ("gap_ms", ctypes.c_float),
                ("enqueue_ms", ctypes.c_double), ("first_seen_ms", ctypes.c_double),
                ("last_seen_ms", ctypes.c_double), ("query_ms", ctypes.c_double), ("wall_ms", ctypes.c_double),
                ("spin_rc", ctypes.c_int32), ("device_flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 6)]

    def as_dict(self) -> dict:
        return {k: (round(getattr(self, k), 4) if isinstance(getattr(self, k), float) else getattr(self, k))
                for k, _ in self._fields_ if k != "reserved"}


class FieldDef(ctypes.Structure):
    """bt_field_def: one FieldDefinition of a user protocol table."""
    _fields_ = [("offset", ctypes.c_uint64), ("length", ctypes.c_uint64), ("type", ctypes.c_uint32),
                ("endianness", ctypes.c_uint32)]


class ExtractOut(ctypes.Structure):
    _fields_ = [("status", ctypes.c_void_p), ("values", ctypes.c_void_p), ("image", ctypes.c_void_p),
                ("n_cap", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


# FieldType (reference include/parser/FieldDefinition.hpp:16-35)
(FT_UINT8, FT_UINT16, FT_UINT32, FT_UINT64, FT_INT8, FT_INT16, FT_INT32, FT_INT64, FT_FLOAT32, FT_FLOAT64,
 FT_BYTES, FT_STRING, FT_BOOLEAN, FT_MAC, FT_IPV4, FT_IPV6, FT_TIMESTAMP, FT_CUSTOM) = range(18)


def field_table(fields):
    """fields: (offset, length, type, endianness) tuples -> (bt_field_def array, n)."""
    arr = (FieldDef * max(1, len(fields)))()
    for i, (o, ln, t, e) in enumerate(fields):
        arr[i] = FieldDef(int(o), int(ln), int(t), int(e))
    return arr, len(fields)


def proto_span(fields) -> int:
    arr, n = field_table(fields)
    span = ctypes.c_uint64(0)
    _check(lib().bt_proto_span(arr, n, ctypes.byref(span)))
    return span.value


class SplitCost(ctypes.Structure):
    """bt_split_cost: packet cost = round_up(min(len, window), align) + fixed."""
    _fields_ = [("window", ctypes.c_uint32), ("align", ctypes.c_uint32), ("fixed", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]

    def as_tuple(self):
        return (self.window, self.align, self.fixed)


class Placement(ctypes.Structure):
    """bt_placement: where a context's host work runs (bt_context_placement)."""
    _fields_ = [("numa_node", ctypes.c_int32), ("pinned_cpus", ctypes.c_uint32), ("pool_threads", ctypes.c_uint32),
                ("staging_node", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 4)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class Tpv3Ring(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("block_size", ctypes.c_uint64), ("n_blocks", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class RingStageOpts(ctypes.Structure):
    """bt_ring_stage_opts (include/beatrice_gpu.h)."""
    _fields_ = [("batch_blocks", ctypes.c_uint32), ("gather", ctypes.c_uint32), ("in_place_every", ctypes.c_uint32),
                ("in_place_blocks", ctypes.c_uint32)]


EXPORTS = [
    "bt_abi_version", "bt_last_error", "bt_create", "bt_destroy", "bt_device_count", "bt_context_device",
    "bt_filter_compile",
    "bt_filter_program", "bt_filter_compile_host", "bt_reserve", "bt_parse_filter_device",
    "bt_parse_filter_device_async",
    "bt_parse_filter", "bt_parse_filter_ptrs", "bt_host_stage_bytes", "bt_host_register", "bt_host_unregister", "bt_dev_malloc", "bt_dev_free", "bt_memcpy_h2d", "bt_memcpy_d2h", "bt_memset_d",
    "bt_synchronize", "bt_host_parallel", "bt_stream_create", "bt_stream_synchronize", "bt_stream_destroy", "bt_time_device", "bt_time_device_ex", "bt_time_device2", "bt_proto_span", "bt_extract_device", "bt_extract", "bt_time_extract_ex", "bt_time_extract2", "bt_record_gather", "bt_record_gather_planes",
    "bt_ring_walk_tpv3", "bt_ring_release_tpv3", "bt_ring_walk_tpv3_gpu",
    "bt_payload_dfa_compile", "bt_payload_dfa_compile_ex", "bt_payload_dfa_search", "bt_payload_dfa_eval",
    "bt_format_records", "bt_format_records_to",
    "bt_record_unpack", "bt_record_slabs", "bt_ring_gather_tpv3", "bt_ring_gather_dense_tpv3",
    "bt_ring_gather_lean_tpv3", "bt_ring_stage_tpv3", "bt_ring_stage_tpv3_ex", "bt_filter_resume_device",
    "bt_group_create", "bt_group_destroy", "bt_group_size", "bt_group_member", "bt_group_filter_compile",
    "bt_group_parse_filter", "bt_group_parse_filter_ptrs", "bt_group_split",
    "bt_group_split_cost", "bt_group_cost", "bt_group_thread_budget", "bt_group_host_register",
    "bt_group_host_unregister", "bt_group_parse_filter_mapped", "bt_context_placement", "bt_node_cpus",
    "bt_usable_cpus", "bt_extract_host", "bt_filter_dfa_pool", "bt_group_split_plan",
    "bt_group_host_parallel", "bt_pass_pack_device", "bt_pcap_index", "bt_pcap_filter", "bt_time_pass_pack",
    "bt_time_copy_d2d", "bt_tally_device", "bt_time_tally", "bt_time_tally_host",
    "bt_flow_fanout_device", "bt_flow_hash_host", "bt_time_fanout", "bt_time_fanout_host",
    "bt_flow_table_scratch_bytes", "bt_flow_table_device", "bt_flow_table_host", "bt_time_flow_table",
    "bt_time_flow_table_host",
    "bt_flow_track_layout", "bt_flow_track_scratch_bytes", "bt_flow_track_expire_scratch_bytes",
    "bt_flow_track_init_device", "bt_flow_track_update_device", "bt_flow_track_expire_device",
    "bt_flow_track_init_host", "bt_flow_track_update_host", "bt_flow_track_expire_host", "bt_flow_track_forget",
    "bt_time_flow_track", "bt_time_flow_track_host",
    "bt_flow_tcp_update_device", "bt_flow_tcp_update_host", "bt_flow_tcp_state", "bt_time_flow_tcp",
    "bt_flow_track_expire_tcp_scratch_bytes", "bt_flow_track_expire_tcp_device", "bt_flow_track_expire_tcp_host",
    "bt_flow_track_top_scratch_bytes", "bt_flow_track_top_device", "bt_flow_track_top_host", "bt_time_flow_top",
    "bt_time_flow_top_host",
    "bt_flow_track_hosts_scratch_bytes", "bt_flow_track_hosts_device", "bt_flow_track_hosts_host", "bt_time_flow_hosts",
    "bt_time_flow_hosts_host",
    "bt_flow_stat_update_device", "bt_flow_stat_update_host", "bt_flow_stat_rtt", "bt_time_flow_stat",
    "bt_flow_track_side_move_scratch_bytes", "bt_flow_track_side_move_device", "bt_flow_track_side_move_host",
    "bt_flow_mark_update_device", "bt_flow_mark_update_host", "bt_flow_mark_select_device", "bt_flow_mark_select_host",
    "bt_time_flow_mark",
    "bt_flow_seq_scratch_bytes", "bt_flow_seq_device", "bt_flow_seq_host", "bt_time_flow_seq",
    "bt_flow_stream_compile", "bt_flow_stream_scratch_bytes", "bt_flow_stream_device", "bt_flow_stream_host",
    "bt_time_flow_stream",
    "bt_flow_tcpseq_scratch_bytes", "bt_flow_tcpseq_device", "bt_flow_tcpseq_host", "bt_time_flow_tcpseq",
    "bt_flow_reasm_scratch_bytes", "bt_flow_reasm_device", "bt_flow_reasm_host", "bt_time_flow_reasm",
    "bt_flow_follow_scratch_bytes", "bt_flow_follow_device", "bt_flow_follow_host", "bt_time_flow_follow",
]

DEST_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)   # bt_format_records_to's dest

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: the gfx950 extension was not built "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int32
    sig = {
        "bt_abi_version": (ctypes.c_int, []),
        "bt_last_error": (ctypes.c_char_p, []),
        "bt_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(Opts), ctypes.POINTER(vp)]),
        "bt_destroy": (None, [vp]),
        "bt_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
        "bt_context_device": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, u32]),
        "bt_filter_compile": (ctypes.c_int, [vp, ctypes.POINTER(FilterDesc), u32]),
        "bt_filter_program": (ctypes.c_int, [vp, ctypes.POINTER(FilterSlot), u32, ctypes.POINTER(u32)]),
        "bt_filter_compile_host": (ctypes.c_int, [ctypes.POINTER(FilterDesc), u32, ctypes.POINTER(FilterSlot),
                                                  u32, ctypes.POINTER(u32)]),
        "bt_reserve": (ctypes.c_int, [vp, u32]),
        "bt_parse_filter_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), ctypes.POINTER(Outputs), vp]),
        "bt_filter_resume_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), ctypes.POINTER(Outputs), vp]),
        "bt_pass_pack_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(PackOpts),
                                               ctypes.POINTER(PackOut), vp]),
        "bt_time_pass_pack": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(PackOpts),
                                             ctypes.POINTER(PackOut), u32, vp]),
        "bt_time_copy_d2d": (ctypes.c_int, [vp, vp, vp, u64, u32, vp]),
        "bt_tally_device": (ctypes.c_int, [vp, vp, u32, ctypes.POINTER(Batch), vp, u32, u32, vp, vp]),
        "bt_time_tally": (ctypes.c_int, [vp, vp, u32, ctypes.POINTER(Batch), vp, u32, u32, vp, u32, vp]),
        "bt_time_tally_host": (ctypes.c_int, [vp, vp, u32, u32, vp, vp, vp]),
        "bt_flow_fanout_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(FanoutOpts),
                                                 ctypes.POINTER(FanoutOut), vp]),
        "bt_flow_hash_host": (ctypes.c_int, [vp, u32, ctypes.POINTER(FanoutOpts), ctypes.POINTER(u32),
                                             ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "bt_time_fanout": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(FanoutOpts),
                                          ctypes.POINTER(FanoutOut), u32, vp]),
        "bt_time_fanout_host": (ctypes.c_int, [vp, vp, u32, vp, vp, ctypes.POINTER(FanoutOpts), u32, vp, vp, vp]),
        "bt_flow_table_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(u64)]),
        "bt_flow_table_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(FlowTableOpts), vp, u64,
                                                ctypes.POINTER(FlowTableOut), vp]),
        "bt_flow_table_host": (ctypes.c_int, [vp, u64, vp, u32, vp, ctypes.POINTER(FlowTableOpts), vp, vp,
                                              ctypes.POINTER(FlowTableResult)]),
        "bt_time_flow_table": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(FlowTableOpts), vp, u64,
                                              ctypes.POINTER(FlowTableOut), u32, vp]),
        "bt_time_flow_table_host": (ctypes.c_int, [vp, vp, u32, vp, u64, vp, ctypes.POINTER(FlowTableOpts), u32, vp, vp,
                                                   ctypes.POINTER(FlowTableResult)]),
        "bt_flow_track_layout": (ctypes.c_int, [u32, u32, ctypes.POINTER(FlowTrackSizes)]),
        "bt_flow_track_scratch_bytes": (ctypes.c_int, [u32, ctypes.POINTER(u64)]),
        "bt_flow_track_expire_scratch_bytes": (ctypes.c_int, [u32, ctypes.POINTER(u64)]),
        "bt_flow_track_init_device": (ctypes.c_int, [vp, vp, u64, ctypes.POINTER(FlowTrackOpts), vp]),
        "bt_flow_track_update_device": (ctypes.c_int, [vp, vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(FlowTrackUpdate), vp, u64,
                                                       ctypes.POINTER(FlowTrackOut), vp]),
        "bt_flow_track_expire_device": (ctypes.c_int, [vp, vp, u64, u64, vp, u64, ctypes.POINTER(FlowTrackExpireOut), vp]),
        "bt_flow_track_forget": (ctypes.c_int, [vp]),
        "bt_flow_track_init_host": (ctypes.c_int, [vp, u64, ctypes.POINTER(FlowTrackOpts)]),
        "bt_flow_track_update_host": (ctypes.c_int, [vp, u64, vp, u64, vp, u32, vp, ctypes.POINTER(FlowTrackUpdate), vp,
                                                     ctypes.POINTER(FlowTrackResult)]),
        "bt_flow_track_expire_host": (ctypes.c_int, [vp, u64, u64, u64, ctypes.POINTER(FlowTrackExpireOut)]),
        "bt_time_flow_track": (ctypes.c_int, [vp, vp, ctypes.POINTER(Batch), vp, ctypes.POINTER(FlowTrackUpdate), vp, u64,
                                              ctypes.POINTER(FlowTrackOut), u32, vp]),
        "bt_time_flow_track_host": (ctypes.c_int, [vp, vp, u32, vp, u64, u64, u32, vp, vp, ctypes.POINTER(FlowTrackResult)]),
        "bt_flow_tcp_update_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, vp, u32, vp, vp]),
        "bt_flow_tcp_update_host": (ctypes.c_int, [vp, u64, vp, u32, vp, u32, vp, u32, vp]),
        "bt_flow_tcp_state": (ctypes.c_int, [u32, u32, u32]),
        "bt_time_flow_tcp": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, vp, u32, vp, u32, vp]),
        "bt_flow_track_expire_tcp_scratch_bytes": (ctypes.c_int, [u32, ctypes.POINTER(u64)]),
        "bt_flow_track_expire_tcp_device": (ctypes.c_int, [vp, vp, u64, u64, ctypes.POINTER(FlowTrackExpireTcp), vp, u64,
                                                           ctypes.POINTER(FlowTrackExpireOut), vp]),
        "bt_flow_track_expire_tcp_host": (ctypes.c_int, [vp, u64, u64, u64, ctypes.POINTER(FlowTrackExpireTcp),
                                                         ctypes.POINTER(FlowTrackExpireOut)]),
        "bt_flow_track_top_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(u64)]),
        "bt_flow_track_top_device": (ctypes.c_int, [vp, vp, ctypes.POINTER(FlowTopOpts), vp, vp, u64, ctypes.POINTER(FlowTopOut), vp]),
        "bt_flow_track_top_host": (ctypes.c_int, [vp, u64, ctypes.POINTER(FlowTopOpts), vp, ctypes.POINTER(FlowTopOut)]),
        "bt_time_flow_top": (ctypes.c_int, [vp, vp, ctypes.POINTER(FlowTopOpts), vp, vp, u64, ctypes.POINTER(FlowTopOut), u32, vp]),
        "bt_time_flow_top_host": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, vp, ctypes.POINTER(u64)]),
        "bt_flow_track_hosts_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(u64)]),
        "bt_flow_track_hosts_device": (ctypes.c_int, [vp, vp, ctypes.POINTER(FlowHostsOpts), vp, vp, u64, ctypes.POINTER(FlowHostsOut), vp]),
        "bt_flow_track_hosts_host": (ctypes.c_int, [vp, u64, ctypes.POINTER(FlowHostsOpts), vp, ctypes.POINTER(FlowHostsOut)]),
        "bt_time_flow_hosts": (ctypes.c_int, [vp, vp, ctypes.POINTER(FlowHostsOpts), vp, vp, u64, ctypes.POINTER(FlowHostsOut), u32, vp]),
        "bt_time_flow_hosts_host": (ctypes.c_int, [vp, vp, u32, vp, ctypes.POINTER(FlowHostsOpts), u32, vp, vp, vp, vp]),
        "bt_flow_stat_update_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, ctypes.POINTER(FlowTrackUpdate), vp, u32, vp, vp]),
        "bt_flow_stat_update_host": (ctypes.c_int, [vp, u64, vp, u32, vp, u32, ctypes.POINTER(FlowTrackUpdate), vp, u32, vp]),
        "bt_flow_stat_rtt": (ctypes.c_int, [vp, vp]),
        "bt_time_flow_stat": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, ctypes.POINTER(FlowTrackUpdate), vp, u32, vp, u32, vp]),
        "bt_flow_track_side_move_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(u64)]),
        "bt_flow_track_side_move_device": (ctypes.c_int, [vp, ctypes.POINTER(FlowSideMove), vp, u64, vp]),
        "bt_flow_track_side_move_host": (ctypes.c_int, [ctypes.POINTER(FlowSideMove)]),
        "bt_flow_mark_update_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, ctypes.POINTER(FlowMarkUpdate), vp, u32, vp, vp]),
        "bt_flow_mark_update_host": (ctypes.c_int, [vp, u32, vp, vp, ctypes.POINTER(FlowMarkUpdate), vp, u32, vp]),
        "bt_flow_mark_select_device": (ctypes.c_int, [vp, vp, u32, vp, u32, ctypes.POINTER(FlowMarkSelectOpts), vp, vp, vp, vp]),
        "bt_flow_mark_select_host": (ctypes.c_int, [vp, u32, vp, u32, ctypes.POINTER(FlowMarkSelectOpts), vp, vp, vp]),
        "bt_time_flow_mark": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, ctypes.POINTER(FlowMarkUpdate), vp, u32, vp,
                                             ctypes.POINTER(FlowMarkSelectOpts), vp, vp, vp, u32, vp, vp]),
        "bt_flow_seq_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(ctypes.c_uint64)]),
        "bt_flow_seq_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, ctypes.POINTER(FlowSeqOpts), vp, u32,
                                              ctypes.POINTER(FlowSeqOut), vp, ctypes.c_uint64, vp, vp]),
        "bt_flow_seq_host": (ctypes.c_int, [vp, u32, vp, vp, ctypes.POINTER(FlowSeqOpts), vp, u32, ctypes.POINTER(FlowSeqOut), vp]),
        "bt_time_flow_seq": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, ctypes.POINTER(FlowSeqOpts), vp, u32,
                                            ctypes.POINTER(FlowSeqOut), vp, ctypes.c_uint64, vp, u32, vp, vp]),
        "bt_flow_stream_compile": (ctypes.c_int, [ctypes.c_char_p, vp, u32, ctypes.POINTER(u32), vp]),
        "bt_flow_stream_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(ctypes.c_uint64)]),
        "bt_flow_stream_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, u32, vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                                 ctypes.POINTER(FlowStreamOut), vp]),
        "bt_flow_stream_host": (ctypes.c_int, [vp, ctypes.c_uint64, vp, u32, vp, vp, u32, vp, u32, vp, u32,
                                               ctypes.POINTER(FlowStreamOut)]),
        "bt_time_flow_stream": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, u32, vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                               ctypes.POINTER(FlowStreamOut), u32, vp, vp]),
        "bt_flow_tcpseq_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(ctypes.c_uint64)]),
        "bt_flow_tcpseq_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                                 ctypes.POINTER(FlowTcpseqOut), vp]),
        "bt_flow_tcpseq_host": (ctypes.c_int, [vp, ctypes.c_uint64, vp, u32, vp, vp, u32, vp, u32, ctypes.POINTER(FlowTcpseqOut)]),
        "bt_time_flow_tcpseq": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                               ctypes.POINTER(FlowTcpseqOut), u32, vp, vp]),
        "bt_flow_reasm_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(ctypes.c_uint64)]),
        "bt_flow_reasm_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                                ctypes.POINTER(FlowReasmOut), vp]),
        "bt_flow_reasm_host": (ctypes.c_int, [vp, ctypes.c_uint64, vp, u32, vp, vp, vp, u32, vp, u32, vp, u32,
                                              ctypes.POINTER(FlowReasmOut)]),
        "bt_time_flow_reasm": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                              ctypes.POINTER(FlowReasmOut), u32, vp, vp]),
        "bt_flow_follow_scratch_bytes": (ctypes.c_int, [u32, u32, ctypes.POINTER(ctypes.c_uint64)]),
        "bt_flow_follow_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                                 ctypes.POINTER(FlowReasmOut), ctypes.POINTER(FlowFollowOut), vp]),
        "bt_flow_follow_host": (ctypes.c_int, [vp, ctypes.c_uint64, vp, u32, vp, vp, vp, u32, vp, u32, vp, u32,
                                               ctypes.POINTER(FlowReasmOut), ctypes.POINTER(FlowFollowOut)]),
        "bt_time_flow_follow": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, ctypes.c_uint64,
                                               ctypes.POINTER(FlowReasmOut), ctypes.POINTER(FlowFollowOut), u32, vp, vp]),
        "bt_pcap_index": (ctypes.c_int, [vp, u64, ctypes.POINTER(PcapInfo), vp, u64, ctypes.POINTER(u64)]),
        "bt_pcap_filter": (ctypes.c_int, [vp, vp, u64, vp, u64, ctypes.POINTER(PcapResult)]),
        "bt_parse_filter_device_async": (ctypes.c_int, [vp, ctypes.POINTER(Batch), ctypes.POINTER(Outputs), vp,
                                                        vp]),
        "bt_parse_filter": (ctypes.c_int, [vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "bt_parse_filter_ptrs": (ctypes.c_int, [vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "bt_host_stage_bytes": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(u32)]),
        "bt_host_register": (ctypes.c_int, [vp, vp, u64, ctypes.POINTER(vp)]),
        "bt_host_unregister": (ctypes.c_int, [vp, vp]),
        "bt_dev_malloc": (ctypes.c_int, [vp, u64, ctypes.POINTER(vp)]),
        "bt_dev_free": (ctypes.c_int, [vp, vp]),
        "bt_memcpy_h2d": (ctypes.c_int, [vp, vp, vp, u64]),
        "bt_memcpy_d2h": (ctypes.c_int, [vp, vp, vp, u64]),
        "bt_memset_d": (ctypes.c_int, [vp, vp, ctypes.c_int, u64]),
        "bt_synchronize": (ctypes.c_int, [vp]),
        "bt_stream_create": (ctypes.c_int, [vp, ctypes.POINTER(vp)]),
        "bt_stream_synchronize": (ctypes.c_int, [vp, vp]),
        "bt_stream_destroy": (ctypes.c_int, [vp, vp]),
        "bt_time_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), ctypes.POINTER(Outputs), u32,
                                          ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
        "bt_time_device_ex": (ctypes.c_int, [vp, ctypes.POINTER(Batch), ctypes.POINTER(Outputs), u32,
                                             ctypes.POINTER(Timing)]),
        "bt_time_device2": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, u32, u32, ctypes.POINTER(Timing)]),
        "bt_proto_span": (ctypes.c_int, [vp, u32, ctypes.POINTER(u64)]),
        "bt_extract_device": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, ctypes.POINTER(ExtractOut), vp]),
        "bt_extract": (ctypes.c_int, [vp, vp, vp, u32, vp, u32, vp, vp, vp]),
        "bt_extract_host": (ctypes.c_int, [vp, vp, u32, vp, u32, vp, vp, vp]),
        "bt_filter_dfa_pool": (ctypes.c_int, [vp, vp, u32, ctypes.POINTER(u32)]),
        "bt_time_extract_ex": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, ctypes.POINTER(ExtractOut), u32,
                                              ctypes.POINTER(Timing)]),
        "bt_time_extract2": (ctypes.c_int, [vp, ctypes.POINTER(Batch), vp, u32, ctypes.POINTER(ExtractOut), u32, u32,
                                            ctypes.POINTER(Timing)]),
        "bt_record_gather": (None, [vp, u32, u32, vp]),
        "bt_record_gather_planes": (None, [vp, u32, u32, vp]),
        "bt_ring_walk_tpv3": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), u32, u32, vp, u32,
                                             ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "bt_ring_release_tpv3": (ctypes.c_int, [ctypes.POINTER(Tpv3Ring), u32, u32]),
        "bt_ring_walk_tpv3_gpu": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), vp, u32, u32, vp, u32,
                                                 ctypes.POINTER(u32), ctypes.POINTER(u32), vp, vp]),
        "bt_ring_gather_tpv3": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), u32, u32, vp, vp, u32,
                                               ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "bt_ring_gather_dense_tpv3": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), u32, u32, vp, vp, vp, u32,
                                                     ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "bt_ring_gather_lean_tpv3": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), u32, u32, vp, vp, vp, u32,
                                                     ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "bt_ring_stage_tpv3": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), u32, u32, ctypes.POINTER(RingStageOpts),
                                              vp, vp, vp, vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]),
        "bt_ring_stage_tpv3_ex": (ctypes.c_int, [vp, ctypes.POINTER(Tpv3Ring), u32, u32, ctypes.POINTER(RingStageOpts),
                                                 u32, vp, vp, vp, vp, vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32),
                                                 ctypes.POINTER(u32)]),
        "bt_payload_dfa_compile": (ctypes.c_int, [ctypes.c_char_p, vp, u32, ctypes.POINTER(u32)]),
        "bt_payload_dfa_compile_ex": (ctypes.c_int, [ctypes.c_char_p, u32, vp, u32, ctypes.POINTER(u32)]),
        "bt_payload_dfa_search": (ctypes.c_int, [vp, vp, u32]),
        "bt_payload_dfa_eval": (ctypes.c_int, [vp, vp, u32]),
        "bt_format_records": (ctypes.c_int, [vp, vp, u32, u32, vp, u64, ctypes.POINTER(u64), vp]),
        "bt_format_records_to": (ctypes.c_int, [vp, vp, u32, u32, DEST_FN, vp, ctypes.POINTER(u64), vp]),
        "bt_record_unpack": (ctypes.c_int, [vp, vp, u32, u32, u32, vp, ctypes.POINTER(u64)]),
        "bt_record_slabs": (u32, [vp]),
        "bt_group_create": (ctypes.c_int, [vp, u32, ctypes.POINTER(Opts), ctypes.POINTER(vp)]),
        "bt_group_destroy": (None, [vp]),
        "bt_group_size": (u32, [vp]),
        "bt_group_member": (vp, [vp, u32]),
        "bt_group_filter_compile": (ctypes.c_int, [vp, ctypes.POINTER(FilterDesc), u32]),
        "bt_group_parse_filter": (ctypes.c_int, [vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "bt_group_parse_filter_ptrs": (ctypes.c_int, [vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "bt_group_split": (ctypes.c_int, [vp, u32, u32, vp]),
        "bt_group_split_cost": (ctypes.c_int, [vp, u32, u32, ctypes.POINTER(SplitCost), vp]),
        "bt_group_split_plan": (ctypes.c_int, [vp, u32, u32, ctypes.POINTER(SplitCost), vp]),
        "bt_group_host_parallel": (ctypes.c_int, [vp, vp, vp]),
        "bt_group_cost": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, u32, ctypes.POINTER(SplitCost)]),
        "bt_group_thread_budget": (ctypes.c_int, [u32, u32, u32, ctypes.POINTER(u32)]),
        "bt_group_host_register": (ctypes.c_int, [vp, vp, u64]),
        "bt_group_host_unregister": (ctypes.c_int, [vp, vp]),
        "bt_group_parse_filter_mapped": (ctypes.c_int, [vp, ctypes.POINTER(Batch), ctypes.POINTER(Outputs)]),
        "bt_context_placement": (ctypes.c_int, [vp, ctypes.POINTER(Placement)]),
        "bt_node_cpus": (ctypes.c_int, [ctypes.c_int, vp, u32, ctypes.POINTER(u32)]),
        "bt_usable_cpus": (u32, []),
    }
    for name, (res, args) in sig.items():
        if not hasattr(L, name):   # an older build under BT_LIB_PATH (A/B runs); tests check EXPORTS
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _ = i32
    have = L.bt_abi_version()
    if have < ABI_VERSION:
        msg = f"{LIB_PATH}: C-ABI version {have}, this binding needs {ABI_VERSION} (rebuild the library)"
        if not os.environ.get("BT_LIB_PATH"):
            raise RuntimeError(msg)
        import sys   # an older build under BT_LIB_PATH (A/B runs): what it lacks fails when called
        print(f"beatrice_amd.abi: warning: {msg}", file=sys.stderr)
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise BtError(rc, lib().bt_last_error().decode(errors="replace"))


def filter_descs(filters):
    """filters: list of dicts {type, expr, enabled=1, priority=0, custom=0}."""
    arr = (FilterDesc * max(1, len(filters)))()
    keep = []
    for i, f in enumerate(filters):
        e = f.get("expr", "").encode()
        keep.append(e)
        arr[i] = FilterDesc(f["type"], e, int(f.get("enabled", 1)), int(f.get("priority", 0)),
                            int(bool(f.get("custom", 0))))
    arr._keep = keep
    return arr


def compile_host(filters):
    """Host-only compile (no GPU needed): list of FilterSlot in evaluation order."""
    arr = filter_descs(filters)
    out = (FilterSlot * BT_MAX_FILTERS)()
    n = ctypes.c_uint32(0)
    _check(lib().bt_filter_compile_host(arr, len(filters), out, BT_MAX_FILTERS, ctypes.byref(n)))
    return [out[i] for i in range(n.value)]


def _byte_view(buf) -> np.ndarray:
    """A contiguous uint8 view (or copy) of bytes / bytearray / a numpy array."""
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(buf, np.uint8)


def pcap_index(buf, count_only: bool = False):
    """bt_pcap_index (host only) over a classic pcap file held in memory: (info dict, descriptors)
    with desc[i] = offset of record i's data | incl_len << 48, up to the last whole record
    (info["truncated"] = 1 when bytes follow it). count_only: (info, n) without descriptors."""
    a = _byte_view(buf)
    keep = a if len(a) else np.zeros(1, np.uint8)
    info, n = PcapInfo(), ctypes.c_uint64(0)
    _check(lib().bt_pcap_index(keep.ctypes.data, len(a), ctypes.byref(info), None, 0, ctypes.byref(n)))
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    if count_only:
        return d, int(n.value)
    desc = np.zeros(max(1, n.value), np.uint64)
    _check(lib().bt_pcap_index(keep.ctypes.data, len(a), ctypes.byref(info), desc.ctypes.data, n.value,
                               ctypes.byref(n)))
    return d, desc[:n.value]


FMT_JSON, FMT_XML, FMT_CSV, FMT_HUMAN = range(4)


def format_records_once(records: np.ndarray, fmt: int = FMT_JSON, ctx: "Context | None" = None) -> bytes:
    """bt_format_records_to: the same text as format_records, formatted once."""
    recs = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 96)
    held = {}

    def dest(_user, nbytes):
        held["buf"] = np.empty(max(1, nbytes), np.uint8)
        return held["buf"].ctypes.data

    cb = DEST_FN(dest)
    need = ctypes.c_uint64(0)
    _check(lib().bt_format_records_to(ctx.h if ctx is not None else None, recs.ctypes.data, len(recs), fmt, cb,
                                      None, ctypes.byref(need), None))
    return held["buf"][:need.value].tobytes() if "buf" in held else b""


def format_records(records: np.ndarray, fmt: int = FMT_JSON, ctx: "Context | None" = None,
                   offsets: bool = False):
    """bt_format_records over host bt_rec (REC_DTYPE or (n, 96) u8): the reference
    ParseResult text of every walked layer. Returns bytes (and the n+1 packet offsets)."""
    recs = np.ascontiguousarray(records).view(np.uint8).reshape(-1, 96)
    n = len(recs)
    need = ctypes.c_uint64(0)
    h = ctx.h if ctx is not None else None
    _check(lib().bt_format_records(h, recs.ctypes.data, n, fmt, None, 0, ctypes.byref(need), None))
    out = np.empty(max(1, need.value), np.uint8)
    off = np.empty(n + 1, np.uint64) if offsets else None
    _check(lib().bt_format_records(h, recs.ctypes.data, n, fmt, out.ctypes.data, need.value, ctypes.byref(need),
                                   off.ctypes.data if offsets else None))
    text = out[:need.value].tobytes()
    return (text, off) if offsets else text


def device_count() -> int:
    n = ctypes.c_int(0)
    lib().bt_device_count(ctypes.byref(n))
    return n.value


class DeviceBuffer:
    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p(0)
        _check(lib().bt_dev_malloc(ctx.h, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        assert offset >= 0 and offset + arr.nbytes <= self.nbytes
        _check(lib().bt_memcpy_h2d(self.ctx.h, self.ptr + offset, arr.ctypes.data, arr.nbytes))

    def download(self, arr: np.ndarray):
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        _check(lib().bt_memcpy_d2h(self.ctx.h, arr.ctypes.data, self.ptr, arr.nbytes))
        return arr

    def zero(self):
        _check(lib().bt_memset_d(self.ctx.h, self.ptr, 0, self.nbytes))

    def free(self):
        """hipFree waits for the device, so an asynchronous kernel fault is reported here:
        raise it (a swallowed fault resurfaces at some later, unrelated call)."""
        if self.ptr:
            if not self.ctx.h:
                raise BtError(1, "DeviceBuffer.free after its context was closed")
            p, self.ptr = self.ptr, None
            _check(lib().bt_dev_free(self.ctx.h, p))

    def __del__(self):
        try:
            self.free()
        except Exception as e:   # cannot raise from a finaliser: say so loudly
            import sys
            print(f"beatrice_amd.abi: DeviceBuffer finaliser: {e}", file=sys.stderr, flush=True)


class Context:
    """One bt_ctx on one device."""

    def __init__(self, device: int = 0, host_chunk_packets: int = 0, grid_waves: int = 0, flags: int = 0,
                 host_threads: int = 0, host_chunk_bytes: int = 0):
        opts = Opts()
        opts.host_threads = host_threads
        opts.host_chunk_packets = host_chunk_packets
        opts.host_chunk_bytes = host_chunk_bytes
        opts.grid_waves = grid_waves
        opts.flags = flags
        h = ctypes.c_void_p(0)
        _check(lib().bt_create(device, ctypes.byref(opts), ctypes.byref(h)))
        self.h = h.value
        self.device = device
        self.flags = flags

    def close(self):
        if self.h:
            lib().bt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_id(self) -> tuple[int, str]:
        """(HIP ordinal, PCI bus id) of the context's device (bt_context_device)."""
        d = ctypes.c_int(-1)
        bus = ctypes.create_string_buffer(64)
        _check(lib().bt_context_device(self.h, ctypes.byref(d), bus, 64))
        return d.value, bus.value.decode(errors="replace")

    def compile(self, filters):
        arr = filter_descs(filters)
        _check(lib().bt_filter_compile(self.h, arr, len(filters)))
        return self.program()

    def program(self):
        out = (FilterSlot * BT_MAX_FILTERS)()
        n = ctypes.c_uint32(0)
        _check(lib().bt_filter_program(self.h, out, BT_MAX_FILTERS, ctypes.byref(n)))
        return [out[i] for i in range(n.value)]

    def reserve(self, n: int):
        _check(lib().bt_reserve(self.h, n))

    def placement(self) -> dict:
        """bt_context_placement: NUMA node, pinned CPUs, pool size, staging node."""
        p = Placement()
        _check(lib().bt_context_placement(self.h, ctypes.byref(p)))
        return p.as_dict()

    def register(self, arr: np.ndarray) -> int:
        """Page-lock + map a host array (zero-copy); returns its device alias."""
        p = ctypes.c_void_p(0)
        _check(lib().bt_host_register(self.h, arr.ctypes.data, arr.nbytes, ctypes.byref(p)))
        return p.value

    def unregister(self, arr: np.ndarray):
        _check(lib().bt_host_unregister(self.h, arr.ctypes.data))

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def synchronize(self):
        _check(lib().bt_synchronize(self.h))

    def stream_create(self) -> int:
        """A caller-owned hipStream_t on the context's device (bt_stream_create)."""
        p = ctypes.c_void_p(0)
        _check(lib().bt_stream_create(self.h, ctypes.byref(p)))
        return p.value

    def stream_synchronize(self, stream: int):
        _check(lib().bt_stream_synchronize(self.h, stream))

    def stream_destroy(self, stream: int):
        _check(lib().bt_stream_destroy(self.h, stream))

    def run_device(self, batch: Batch, outs: Outputs, stream=None):
        _check(lib().bt_parse_filter_device(self.h, ctypes.byref(batch), ctypes.byref(outs), stream))

    def resume_device(self, batch: Batch, outs: Outputs, stream=None):
        """bt_filter_resume_device: the second pass over a batch first run with BATCH_PREFIXES.
        `batch` holds the whole frames of the same packets (flags 0), outs.decide the first
        pass's decision bytes (rewritten in place); outs.verdict / pass_idx / n_pass, when set,
        are rebuilt from the final bytes. outs.records must be None."""
        _check(lib().bt_filter_resume_device(self.h, ctypes.byref(batch), ctypes.byref(outs), stream))

    def pass_pack(self, batch: Batch, select_dev, out_bytes, cap: int, total, n_packed, desc=None, lead: int = 0,
                  snap: int = 0, align: int = 1, stream=None):
        """bt_pass_pack_device: the frames of `batch` whose bit is set in the verdict-layout words
        at `select_dev`, packed in packet order into out_bytes[:cap]; record k = lead bytes in
        front of the frame + min(len, snap or len) frame bytes, its slot rounded up to align.
        Every pointer argument is a device-visible address (int or DeviceBuffer); total (u64) and
        n_packed (u32) receive the bytes the selection needs and the records that fit; desc
        (optional) one descriptor per selected packet. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        po = PackOpts(lead, snap, align, 0)
        out = PackOut(ptr(out_bytes), cap, ptr(desc), ptr(total), ptr(n_packed))
        _check(lib().bt_pass_pack_device(self.h, ctypes.byref(batch), ptr(select_dev), ctypes.byref(po),
                                         ctypes.byref(out), stream))

    def tally_device(self, decide_ptr, n: int, out_ptr, frames: "Batch | None" = None, records_ptr=None,
                     n_cap: int = 0, flags: int = 0, stream=None):
        """bt_tally_device: the counts of a device-resident batch into the bt_tally (Tally, 2,304 B
        of device-visible memory, 8-byte aligned) at out_ptr. decide_ptr: the n decision bytes of
        a filter call (any alignment; None for the layer counts alone); frames: the batch, for the
        byte sums (only lengths are read); records_ptr / n_cap: the call's records in the context's
        layout, for the layer counts. flags: TALLY_STOP_AT_THROW, TALLY_ACCUMULATE. Pointers are
        addresses or DeviceBuffers. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        _check(lib().bt_tally_device(self.h, ptr(decide_ptr), n, ctypes.byref(frames) if frames is not None else None,
                                     ptr(records_ptr), n_cap, flags, ptr(out_ptr), stream))

    def flow_fanout_device(self, batch: Batch, opts: "FanoutOpts", result, select=None, hash=None, queue=None,
                           idx=None, select_q=None, stream=None):
        """bt_flow_fanout_device: the packets of `batch` selected by the verdict-layout words at
        `select` (None = all) fanned out to opts.queues queues by RSS flow hash. result: 808 B
        (FanoutResult), 8-byte aligned; hash (n u32), queue (n bytes), idx (n u32: the selected
        indices grouped by queue, ascending inside one) and select_q (queues * ceil(n / 64) words:
        row q is pass_pack's `select` for queue q) are optional. Pointers are addresses or
        DeviceBuffers. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        out = FanoutOut(ptr(hash), ptr(queue), ptr(idx), ptr(select_q), ptr(result))
        _check(lib().bt_flow_fanout_device(self.h, ctypes.byref(batch), ptr(select), ctypes.byref(opts),
                                           ctypes.byref(out), stream))

    def flow_table_device(self, batch: Batch, opts: "FlowTableOpts", scratch, scratch_bytes: int, result, select=None,
                          flow_id=None, flows=None, stream=None):
        """bt_flow_table_device: the flow table of the packets of `batch` selected by the
        verdict-layout words at `select` (None = all). scratch: flow_table_scratch_bytes(n,
        opts.slots) bytes of device memory, 256-byte aligned; result: 72 B (FlowTableResult),
        8-byte aligned; flow_id (n u32) is optional, flows (opts.flow_cap FlowRec) optional when
        flow_cap is 0. Pointers are addresses or DeviceBuffers. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        out = FlowTableOut(ptr(flow_id), ptr(flows), ptr(result))
        _check(lib().bt_flow_table_device(self.h, ctypes.byref(batch), ptr(select), ctypes.byref(opts), ptr(scratch),
                                          scratch_bytes, ctypes.byref(out), stream))

    def flow_track_init(self, state, state_bytes: int, flow_cap: int, flags: int = 0, slots: int = 0, stream=None):
        """bt_flow_track_init_device: an empty tracker in the flow_track_layout(flow_cap, slots)["total"]
        bytes of device memory at `state` (256-byte aligned). flags: FLOWTAB_*, fixed for its life."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        opts = FlowTrackOpts(flags, flow_cap, slots, 0)
        _check(lib().bt_flow_track_init_device(self.h, ptr(state), state_bytes, ctypes.byref(opts), stream))

    @staticmethod
    def flow_track_forget(state):
        """bt_flow_track_forget (host only): the library forgets the tracker at `state`; call it before
        the memory is freed or reused. It holds 256 states."""
        _check(lib().bt_flow_track_forget(state.ptr if isinstance(state, DeviceBuffer) else state))

    def flow_track_update(self, state, batch: Batch, scratch, scratch_bytes: int, result, select=None, ts=None,
                          batch_ts: int = 0, flow_id=None, stream=None):
        """bt_flow_track_update_device: the packets of `batch` selected by the verdict-layout words at
        `select` (None = all) merged into the tracker at `state`. scratch: flow_track_scratch_bytes(n)
        bytes of device memory, 256-byte aligned; result: 64 B (FlowTrackResult), 8-byte aligned; ts:
        n u64 timestamps on the device, or None for the scalar batch_ts; flow_id (n u32) optional.
        Pointers are addresses or DeviceBuffers. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        upd = FlowTrackUpdate(ptr(ts), batch_ts)
        out = FlowTrackOut(ptr(flow_id), ptr(result))
        _check(lib().bt_flow_track_update_device(self.h, ptr(state), ctypes.byref(batch), ptr(select), ctypes.byref(upd),
                                                 ptr(scratch), scratch_bytes, ctypes.byref(out), stream))

    def flow_track_expire(self, state, now: int, idle: int, scratch, scratch_bytes: int, result, expired=None,
                          expired_cap: int = 0, remap=None, stream=None):
        """bt_flow_track_expire_device: the flows with last_ts <= now and now - last_ts > idle leave the
        tracker at `state`, in ascending flow number, into expired[:expired_cap] (FlowTrackRec; None:
        every idle flow is dropped); remap (flow_cap u32, optional): old number -> new number or
        FLOW_ID_EXPIRED. scratch: flow_track_expire_scratch_bytes(flow_cap) bytes; result: 32 B
        (FlowTrackExpireResult). Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        out = FlowTrackExpireOut(ptr(expired), expired_cap, 0, ptr(remap), ptr(result))
        _check(lib().bt_flow_track_expire_device(self.h, ptr(state), now, idle, ptr(scratch), scratch_bytes, ctypes.byref(out),
                                                 stream))

    def flow_tcp_update(self, batch: Batch, flow_id, table_flags: int, tcp, flow_cap: int, result, stream=None):
        """bt_flow_tcp_update_device: the TCP packets of `batch` add their flags byte to the side table
        `tcp` (flow_cap FlowTcpRec on the device, zeroed once by the caller) at their flow number
        flow_id[i] (n u32 from flow_table_device or flow_track_update under the same table_flags).
        result: 32 B (FlowTcpResult), 8-byte aligned. Pointers are addresses or DeviceBuffers.
        Asynchronous on `stream`: enqueue it behind the call that wrote flow_id."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        _check(lib().bt_flow_tcp_update_device(self.h, ctypes.byref(batch), ptr(flow_id), table_flags, ptr(tcp), flow_cap,
                                               ptr(result), stream))

    def flow_stat_update(self, batch: Batch, flow_id, table_flags: int, stat, flow_cap: int, result, ts=None, batch_ts: int = 0,
                         stream=None):
        """bt_flow_stat_update_device: the IP packets of `batch` add protocol, TTL, length, payload and
        handshake stamps to the side table `stat` (flow_cap FlowStatRec on the device, zeroed once by
        the caller) at their flow number flow_id[i] (n u32 from flow_table_device or flow_track_update
        under the same table_flags). A packet's timestamp is ts[i] (device, n u64) or batch_ts.
        result: 32 B (FlowStatResult), 8-byte aligned. Pointers are addresses or DeviceBuffers.
        Asynchronous on `stream`: enqueue it behind the call that wrote flow_id."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        upd = FlowTrackUpdate(ptr(ts), batch_ts)
        _check(lib().bt_flow_stat_update_device(self.h, ctypes.byref(batch), ptr(flow_id), table_flags, ctypes.byref(upd), ptr(stat),
                                                flow_cap, ptr(result), stream))

    def flow_track_side_move(self, side, rec_bytes: int, flow_cap: int, remap, result, scratch, scratch_bytes: int,
                             expired_side=None, expired_cap: int = 0, stream=None):
        """bt_flow_track_side_move_device: the side table `side` (flow_cap records of rec_bytes on the
        device) through the expire that wrote remap (flow_cap u32) and result (its 32 B, on the
        device): survivors to their new number, zeros behind them, the expired flows' records to
        expired_side[:expired_cap] (optional). scratch: flow_track_side_move_scratch_bytes(flow_cap,
        rec_bytes) bytes, 256-byte aligned. Asynchronous on `stream`: enqueue it behind the expire."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        m = FlowSideMove(ptr(side), ptr(expired_side), ptr(remap), ptr(result), rec_bytes, flow_cap, expired_cap, 0)
        _check(lib().bt_flow_track_side_move_device(self.h, ctypes.byref(m), ptr(scratch), scratch_bytes, stream))

    def flow_mark_update(self, batch: Batch, flow_id, hit, mark: int, table, flow_cap: int, result, ts=None, batch_ts: int = 0,
                         stream=None):
        """bt_flow_mark_update_device: the packets of `batch` whose bit is set in `hit` (verdict-layout
        words on the device, out.verdict of a filter call; None = all) raise `mark` on the record of
        their flow number flow_id[i] in `table` (flow_cap FlowMarkRec on the device, zeroed once by
        the caller), with their count, frame lengths and first / last timestamp (ts[i], device, n
        u64, or batch_ts). result: 32 B (FlowMarkResult), 8-byte aligned. Pointers are addresses or
        DeviceBuffers. Asynchronous on `stream`: enqueue it behind the calls that wrote flow_id and hit."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        upd = FlowMarkUpdate(mark, 0, ptr(ts), batch_ts)
        _check(lib().bt_flow_mark_update_device(self.h, ctypes.byref(batch), ptr(flow_id), ptr(hit), ctypes.byref(upd), ptr(table),
                                                flow_cap, ptr(result), stream))

    def flow_mark_select(self, flow_id, n: int, table, flow_cap: int, mask: int, out_select, result, op: int = FLOW_MARK_SET,
                         flags: int = 0, base=None, stream=None):
        """bt_flow_mark_select_device: out_select (ceil(n/64) u64 words on the device, verdict layout)
        = the packets whose flow number flow_id[i] carries a bit of `mask` (with FLOW_MARK_ALL_BITS:
        every bit) in `table`, combined with `base` by a FLOW_MARK_* op (base may be out_select).
        result: 32 B (FlowMarkSelectResult), 8-byte aligned. Asynchronous on `stream`: enqueue it
        behind the call that wrote flow_id and the updates of the table it should see."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        opts = FlowMarkSelectOpts(mask, flags, op, 0)
        _check(lib().bt_flow_mark_select_device(self.h, ptr(flow_id), n, ptr(table), flow_cap, ctypes.byref(opts), ptr(base),
                                                ptr(out_select), ptr(result), stream))

    def flow_seq(self, batch: Batch, flow_id, select, table, flow_cap: int, scratch, scratch_bytes: int, result,
                 max_packets: int = 0, max_bytes: int = 0, flags: int = 0, seq=None, byte_off=None, out_select=None, stream=None):
        """bt_flow_seq_device: the packets of `batch` whose bit is set in `select` (verdict-layout words
        on the device; None = all) and whose flow number flow_id[i] is below flow_cap are numbered
        inside their flow against `table` (flow_cap FlowSeqRec on the device, zeroed once by the
        caller): seq (n u32) and byte_off (n u64) get the flow's packets and bytes before each, and
        out_select (ceil(n/64) u64 words, may be `select`) the packets within max_packets / max_bytes
        per flow (0 = no limit), with FLOW_SEQ_KEEP_UNKEYED also the selected packets without a flow.
        scratch: flow_seq_scratch_bytes(n, flow_cap) bytes, 256-byte aligned. result: 64 B
        (FlowSeqResult), 8-byte aligned. Pointers are addresses or DeviceBuffers. Asynchronous on
        `stream`: enqueue it behind the calls that wrote flow_id and select."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        opts = FlowSeqOpts(max_packets, max_bytes, flags, (ctypes.c_uint32 * 3)(0, 0, 0))
        out = FlowSeqOut(ptr(seq), ptr(byte_off), ptr(out_select))
        _check(lib().bt_flow_seq_device(self.h, ctypes.byref(batch), ptr(flow_id), ptr(select), ctypes.byref(opts), ptr(table),
                                        flow_cap, ctypes.byref(out), ptr(scratch), scratch_bytes, ptr(result), stream))

    def flow_stream(self, batch: Batch, flow_id, select, table_flags: int, pattern, pattern_device, table, flow_cap: int,
                    scratch, scratch_bytes: int, result, hit=None, stream=None):
        """bt_flow_stream_device: the L4 payloads of the packets of `batch` whose bit is set in `select`
        (verdict-layout words on the device; None = all) and whose flow number flow_id[i] is below
        flow_cap are appended to their (flow, direction) streams, and `pattern` (flow_stream_compile's
        blob on the host; pattern_device: a device copy of it, 8-byte aligned) is matched across
        packet and batch boundaries against `table` (flow_cap FlowStreamRec on the device, zeroed
        once by the caller). hit (ceil(n/64) u64 words, may be `select`) gets the packets in which a
        match ends. scratch: flow_stream_scratch_bytes(n, flow_cap) bytes, 256-byte aligned. result:
        64 B (FlowStreamResult), 8-byte aligned. Pointers are addresses or DeviceBuffers.
        Asynchronous on `stream`: enqueue it behind the calls that wrote flow_id and select."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        pat = np.ascontiguousarray(pattern, np.uint8)
        out = FlowStreamOut(ptr(hit), ptr(result), (ctypes.c_uint64 * 2)(0, 0))
        _check(lib().bt_flow_stream_device(self.h, ctypes.byref(batch), ptr(flow_id), ptr(select), table_flags,
                                           pat.ctypes.data if len(pat) else None, ptr(pattern_device), len(pat), ptr(table), flow_cap,
                                           ptr(scratch), scratch_bytes, ctypes.byref(out), stream))

    def flow_tcpseq(self, batch: Batch, flow_id, select, table_flags: int, table, flow_cap: int, scratch, scratch_bytes: int, result,
                    cls=None, off=None, out_select=None, stream=None):
        """bt_flow_tcpseq_device: the TCP segments of the packets of `batch` whose bit is set in `select`
        (verdict-layout words on the device; None = all) and whose flow number flow_id[i] is below
        flow_cap are placed in their (flow, direction) sequence space and classified (TCPSEQ_*)
        against `table` (flow_cap FlowTcpseqRec on the device, zeroed once by the caller). cls (n
        bytes), off (n int64) and out_select (ceil(n/64) u64 words, may be `select`: select & ~OLD,
        the selection to hand to flow_stream) are optional. scratch: flow_tcpseq_scratch_bytes(n,
        flow_cap) bytes, 256-byte aligned. result: 64 B (FlowTcpseqResult), 8-byte aligned. Pointers
        are addresses or DeviceBuffers. Asynchronous on `stream`: enqueue it behind the calls that
        wrote flow_id and select."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        out = FlowTcpseqOut(ptr(cls), ptr(off), ptr(out_select), ptr(result), (ctypes.c_uint64 * 2)(0, 0))
        _check(lib().bt_flow_tcpseq_device(self.h, ctypes.byref(batch), ptr(flow_id), ptr(select), table_flags, ptr(table), flow_cap,
                                           ptr(scratch), scratch_bytes, ctypes.byref(out), stream))

    def flow_reasm(self, batch: Batch, flow_id, select, off, table_flags: int, pattern, pattern_device, table, flow_cap: int,
                   scratch, scratch_bytes: int, result, hit=None, rest=None, stream=None):
        """bt_flow_reasm_device: the TCP segments of the packets of `batch` whose bit is set in `select`
        (verdict-layout words on the device; None = all; the same words flow_tcpseq took), whose
        flow number flow_id[i] is below flow_cap and which flow_tcpseq placed (`off`, n int64 on the
        device) are ordered by sequence position per (flow, direction), trimmed where they overlap,
        and `pattern` (flow_stream_compile's blob; pattern_device its device copy) is matched over
        the bytes in that order against `table` (flow_cap FlowReasmRec on the device, zeroed once by
        the caller). hit and rest (ceil(n/64) u64 words each; either may be `select`) are optional:
        the packets from whose delivered bytes a match ends, and the selection to hand to
        flow_stream for everything that was not placed. scratch: flow_reasm_scratch_bytes(n,
        flow_cap) bytes, 256-byte aligned. result: 64 B (FlowReasmResult), 8-byte aligned. Pointers
        are addresses or DeviceBuffers. Asynchronous on `stream`: enqueue it behind flow_tcpseq."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        pat = np.ascontiguousarray(pattern, np.uint8)
        out = FlowReasmOut(ptr(hit), ptr(rest), ptr(result), (ctypes.c_uint64 * 2)(0, 0))
        _check(lib().bt_flow_reasm_device(self.h, ctypes.byref(batch), ptr(flow_id), ptr(select), ptr(off), table_flags,
                                          pat.ctypes.data if len(pat) else None, ptr(pattern_device), len(pat), ptr(table), flow_cap,
                                          ptr(scratch), scratch_bytes, ctypes.byref(out), stream))

    def flow_follow(self, batch: Batch, flow_id, select, off, table_flags: int, pattern, pattern_device, table, flow_cap: int,
                    scratch, scratch_bytes: int, result, follow_result, out_bytes=None, cap: int = 0, runs=None, run_cap: int = 0,
                    place=None, hit=None, rest=None, stream=None):
        """bt_flow_follow_device: flow_reasm's work on the same arguments and the same `table`, with every
        delivered byte of the call written to out_bytes (cap bytes on the device; None with cap 0: a
        size query) in ascending (flow, direction) and sequence order, the runs between holes to runs
        (run_cap FlowFollowRun on the device) and each packet's output offset to place (n u64 on the
        device; optional). pattern None (then pattern_device None as well): the plain follow, nothing
        is matched and hit is written as zeros. scratch: flow_follow_scratch_bytes(n, flow_cap)
        bytes, 256-byte aligned. result: 64 B (FlowReasmResult); follow_result: 32 B
        (FlowFollowResult); both 8-byte aligned. Pointers are addresses or DeviceBuffers.
        Asynchronous on `stream`: enqueue it behind flow_tcpseq."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        pat = None if pattern is None else np.ascontiguousarray(pattern, np.uint8)
        out = FlowReasmOut(ptr(hit), ptr(rest), ptr(result), (ctypes.c_uint64 * 2)(0, 0))
        fo = FlowFollowOut(ptr(out_bytes), cap, ptr(runs), run_cap, 0, ptr(place), ptr(follow_result), (ctypes.c_uint64 * 2)(0, 0))
        _check(lib().bt_flow_follow_device(self.h, ctypes.byref(batch), ptr(flow_id), ptr(select), ptr(off), table_flags,
                                           pat.ctypes.data if pat is not None and len(pat) else None, ptr(pattern_device),
                                           0 if pat is None else len(pat), ptr(table), flow_cap, ptr(scratch), scratch_bytes,
                                           ctypes.byref(out), ctypes.byref(fo), stream))

    # the host-only forms beside their device forms
    flow_follow_host = staticmethod(flow_follow_host)
    flow_follow_scratch_bytes = staticmethod(flow_follow_scratch_bytes)
    flow_reasm_host = staticmethod(flow_reasm_host)
    flow_reasm_scratch_bytes = staticmethod(flow_reasm_scratch_bytes)
    flow_tcpseq_host = staticmethod(flow_tcpseq_host)
    flow_tcpseq_scratch_bytes = staticmethod(flow_tcpseq_scratch_bytes)
    flow_stream_host = staticmethod(flow_stream_host)
    flow_stream_compile = staticmethod(flow_stream_compile)
    flow_stream_scratch_bytes = staticmethod(flow_stream_scratch_bytes)
    flow_mark_update_host = staticmethod(flow_mark_update_host)
    flow_seq_host = staticmethod(flow_seq_host)
    flow_seq_scratch_bytes = staticmethod(flow_seq_scratch_bytes)
    flow_mark_select_host = staticmethod(flow_mark_select_host)
    flow_stat_update_host = staticmethod(flow_stat_update_host)
    flow_stat_rtt = staticmethod(flow_stat_rtt)
    flow_track_side_move_scratch_bytes = staticmethod(flow_track_side_move_scratch_bytes)
    flow_track_side_move_host = staticmethod(flow_track_side_move_host)

    def flow_track_top(self, state, metric: int, k: int, scratch, scratch_bytes: int, result, top_id=None, top_value=None,
                       top=None, tcp=None, top_tcp=None, stream=None):
        """bt_flow_track_top_device: the k (<= FLOW_TOP_MAX_K) largest flows of the tracker at `state` by
        a FLOW_TOP_* metric, in the order (value descending, flow number ascending), into top_id (u32),
        top_value (u64), top (FlowTrackRec) and top_tcp (FlowTcpRec; needs tcp, the side table of
        flow_cap records, as the TCP metrics do), k entries each and all optional; nothing is written
        at or past n_top. result: 48 B (FlowTopResult), 8-byte aligned. scratch:
        flow_track_top_scratch_bytes(flow_cap, k) bytes, 256-byte aligned. The state and tcp are only
        read. Pointers are addresses or DeviceBuffers. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x   # noqa: E731
        opts = FlowTopOpts(metric, k, (ctypes.c_uint32 * 2)(0, 0))
        out = FlowTopOut(ptr(top_id), ptr(top_value), ptr(top), ptr(top_tcp), ptr(result))
        _check(lib().bt_flow_track_top_device(self.h, ptr(state), ctypes.byref(opts), ptr(tcp), ptr(scratch), scratch_bytes,
                                              ctypes.byref(out), stream))

    def flow_track_hosts(self, state, host_cap: int, scratch, scratch_bytes: int, result, hosts=None, endpoint_host=None,
                         tcp=None, slots: int = 0, stream=None):
        """bt_flow_track_hosts_device: the flows of the tracker at `state` aggregated per address into
        hosts (host_cap FlowHostRec, numbered in order of first appearance; optional with host_cap 0)
        and endpoint_host (2 flow_cap u32, optional: the host number of every flow's two endpoints);
        with tcp (the side table of flow_cap records) the state counts and SYN columns too. result:
        64 B (FlowHostsResult), 8-byte aligned. scratch: flow_track_hosts_scratch_bytes(flow_cap,
        slots) bytes, 256-byte aligned. The state and tcp are only read. Pointers are addresses or
        DeviceBuffers. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x   # noqa: E731
        opts = FlowHostsOpts(slots, host_cap, (ctypes.c_uint32 * 2)(0, 0))
        out = FlowHostsOut(ptr(hosts), ptr(endpoint_host), ptr(result))
        _check(lib().bt_flow_track_hosts_device(self.h, ptr(state), ctypes.byref(opts), ptr(tcp), ptr(scratch), scratch_bytes,
                                                ctypes.byref(out), stream))

    def flow_track_expire_tcp(self, state, now: int, idle: int, closed_idle: int, tcp, scratch, scratch_bytes: int, result,
                              expired=None, expired_cap: int = 0, expired_tcp=None, remap=None, stream=None):
        """bt_flow_track_expire_tcp_device: flow_track_expire with one more way to leave (a flow whose
        TCP state is closed or reset leaves once now - last_ts > closed_idle), and the side table
        `tcp` (flow_cap FlowTcpRec) is renumbered with the records; expired_tcp (expired_cap FlowTcpRec,
        optional) receives the side records of expired[]. scratch:
        flow_track_expire_tcp_scratch_bytes(flow_cap) bytes. Asynchronous on `stream`."""
        ptr = lambda x: x.ptr if isinstance(x, DeviceBuffer) else x  # noqa: E731
        out = FlowTrackExpireOut(ptr(expired), expired_cap, 0, ptr(remap), ptr(result))
        x = FlowTrackExpireTcp(ptr(tcp), ptr(expired_tcp), closed_idle)
        _check(lib().bt_flow_track_expire_tcp_device(self.h, ptr(state), now, idle, ctypes.byref(x), ptr(scratch), scratch_bytes,
                                                     ctypes.byref(out), stream))

    def pcap_filter(self, buf):
        """bt_pcap_filter: the classic pcap file in `buf` through the compiled program. Returns
        (the output pcap as bytes: the input's global header and every passing record, verbatim
        and in order; the result counts as a dict)."""
        a = _byte_view(buf)
        res = PcapResult()
        _check(lib().bt_pcap_filter(self.h, a.ctypes.data if len(a) else None, len(a), None, 0, ctypes.byref(res)))
        out = np.empty(max(1, res.out_bytes), np.uint8)
        _check(lib().bt_pcap_filter(self.h, a.ctypes.data, len(a), out.ctypes.data, res.out_bytes, ctypes.byref(res)))
        return out[:res.out_bytes].tobytes(), res.as_dict()

    def run_device_async(self, batch: Batch, outs: Outputs, stream=None, done_event=None):
        """bt_parse_filter_device_async: the compaction on the context's compaction stream;
        synchronize() (or done_event, a hipEvent_t) before reading pass_idx / n_pass."""
        _check(lib().bt_parse_filter_device_async(self.h, ctypes.byref(batch), ctypes.byref(outs), stream,
                                                  done_event))

    def time_device(self, batch: Batch, outs: Outputs, iters: int):
        a, b = ctypes.c_float(0), ctypes.c_float(0)
        _check(lib().bt_time_device(self.h, ctypes.byref(batch), ctypes.byref(outs), iters, ctypes.byref(a),
                                    ctypes.byref(b)))
        return a.value, b.value

    def time_device_ex(self, batch: Batch, outs: Outputs, iters: int) -> Timing:
        t = Timing()
        _check(lib().bt_time_device_ex(self.h, ctypes.byref(batch), ctypes.byref(outs), iters, ctypes.byref(t)))
        return t

    def time_device2(self, batch: Batch, outs, iters: int, mode: int) -> Timing:
        """bt_time_device2: outs = a list of Outputs (step i writes outs[i % len(outs)])."""
        arr = (Outputs * len(outs))(*outs)
        t = Timing()
        _check(lib().bt_time_device2(self.h, ctypes.byref(batch), ctypes.cast(arr, ctypes.c_void_p), len(outs), iters,
                                     mode, ctypes.byref(t)))
        return t

    def extract_host(self, frames, fields):
        """bt_extract over a list of frames (bytes): (status[n], values[nf, n], image[n, span])."""
        n = len(frames)
        bufs = [np.frombuffer(bytes(f), np.uint8) if len(f) else np.zeros(1, np.uint8) for f in frames]
        ptrs = (ctypes.c_void_p * max(1, n))(*[b.ctypes.data for b in bufs])
        lens = np.array([len(f) for f in frames], np.uint32)
        arr, nf = field_table(fields)
        span = proto_span(fields)
        span = span if span <= 0xFFFF else 0
        status = np.zeros(max(n, 1), np.uint8)
        values = np.zeros(max(1, nf * n), np.uint64)          # field-major, column stride n
        image = np.zeros(max(1, n * span), np.uint8)
        _check(lib().bt_extract(self.h, ptrs, lens.ctypes.data, n, arr, nf, status.ctypes.data,
                                values.ctypes.data if nf else None, image.ctypes.data if span else None))
        return status[:n], values[:nf * n].reshape(nf, n), image[:n * span].reshape(n, span)

    def run_host(self, data: np.ndarray, desc: np.ndarray, records=True, filters=True, outs: dict | None = None):
        """bt_parse_filter over host buffers. Returns dict of numpy outputs. `outs` (from
        host_outputs) reuses output arrays across calls, as a capture loop does."""
        n = len(desc)
        rec, ver, dec, pidx, npass = _host_outputs(n, records, filters, outs)
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        data = np.ascontiguousarray(data)
        desc = np.ascontiguousarray(desc, dtype=np.uint64)
        _check(lib().bt_parse_filter(self.h, p(data), p(desc), n, p(rec), p(ver), p(dec), p(pidx), p(npass)))
        out = {"records": rec, "verdict": ver, "decide": dec}
        if filters:
            out["pass_idx"] = pidx[: int(npass[0])]
            out["n_pass"] = int(npass[0])
        return out


PAGE = 4096


def host_array(shape, dtype=np.uint8) -> np.ndarray:
    """A zeroed array on pages of its own: an anonymous mapping, page-aligned and padded to
    whole pages, that lives as long as the array. Registration (Context.register,
    Group.register) is in whole pages and refuses a range that shares only some of its pages
    with a live registration, so buffers registered side by side (a capture, its
    descriptors, the outputs) are allocated this way, as a UMEM or a ring is."""
    import mmap
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    m = mmap.mmap(-1, max(PAGE, (n + PAGE - 1) // PAGE * PAGE))
    return np.frombuffer(m, dtype=dt, count=n // dt.itemsize).reshape(shape)


def host_copy(arr: np.ndarray) -> np.ndarray:
    """host_array holding a copy of arr."""
    out = host_array(arr.shape, arr.dtype)
    np.copyto(out, arr)
    return out


def host_outputs(n: int, records=True, filters=True) -> dict:
    """Output arrays for run_host calls of n packets, allocated and touched once (a capture
    loop reuses its outputs; fresh arrays would fault their pages in inside every call), each
    on pages of its own (host_array), so any of them may be registered."""
    o = {"records": host_array((n, BT_REC_BYTES), np.uint8) if records else None,
         "verdict": host_array((n + 63) // 64, np.uint64) if filters else None,
         "decide": host_array(n, np.uint8) if filters else None,
         "pass_idx": host_array(max(n, 1), np.uint32) if filters else None,
         "n_pass": host_array(1, np.uint32) if filters else None}
    for a in o.values():
        if a is not None:
            a.fill(0)   # first touch now, outside any timed call
    return o


def _host_outputs(n, records, filters, outs):
    """The output arrays of a run_host call: `outs` (from host_outputs) checked against what
    the call writes — the native side takes bare pointers, so a short or mistyped array would
    be written past its end — or fresh ones."""
    if outs is None:
        outs = host_outputs(n, records, filters)
    else:
        need = {"records": (bool(records), np.uint8, n * BT_REC_BYTES),
                "verdict": (bool(filters), np.uint64, (n + 63) // 64),
                "decide": (bool(filters), np.uint8, n),
                "pass_idx": (bool(filters), np.uint32, max(n, 1)),
                "n_pass": (bool(filters), np.uint32, 1)}
        for k, (want, dt, size) in need.items():
            a = outs.get(k)
            if (a is not None) != want:
                raise ValueError(f"outs[{k!r}]: {'required' if want else 'must be None'} for this call")
            if a is not None and (a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable or a.size < size):
                raise ValueError(f"outs[{k!r}]: need a writable contiguous {np.dtype(dt).name} array of at least "
                                 f"{size} elements, got {a.dtype} x {a.size}")
        # views of this call's part (arrays sized for a larger batch are reused as they are)
        outs = {k: None if outs.get(k) is None else outs[k].reshape(-1)[:size] for k, (_, _, size) in need.items()}
        if outs["records"] is not None:
            outs["records"] = outs["records"].reshape(n, BT_REC_BYTES)
    return outs["records"], outs["verdict"], outs["decide"], outs["pass_idx"], outs["n_pass"]


def group_split(lens: np.ndarray, parts: int, cost=None, plan=False) -> list[tuple[int, int]]:
    """bt_group_split (host only): the members' [lo, hi) packet ranges; cost = (window,
    align, fixed) selects bt_group_split_cost, plan=True bt_group_split_plan (what the
    group's calls use)."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    b = np.zeros(parts + 1, np.uint32)
    lp = lens.ctypes.data if len(lens) else None
    if cost is None:
        _check(lib().bt_group_split(lp, len(lens), parts, b.ctypes.data))
    else:
        c = SplitCost(*[int(x) for x in cost], 0)
        fn = lib().bt_group_split_plan if plan else lib().bt_group_split_cost
        _check(fn(lp, len(lens), parts, ctypes.byref(c), b.ctypes.data))
    return [(int(b[k]), int(b[k + 1])) for k in range(parts)]


def group_thread_budget(members: int, usable: int, requested: int = 0) -> int:
    """bt_group_thread_budget (host only): host threads per member."""
    out = ctypes.c_uint32(0)
    _check(lib().bt_group_thread_budget(members, usable, requested, ctypes.byref(out)))
    return out.value


def node_cpus(node: int) -> list[int]:
    """bt_node_cpus (host only): the CPUs of NUMA node `node` in this process's affinity set."""
    cpus = (ctypes.c_int32 * 4096)()
    n = ctypes.c_uint32(0)
    _check(lib().bt_node_cpus(node, cpus, 4096, ctypes.byref(n)))
    return [cpus[i] for i in range(min(n.value, 4096))]


def usable_cpus() -> int:
    return int(lib().bt_usable_cpus())


class Group:
    """bt_group: one context per device in this process."""

    def __init__(self, devices, host_chunk_packets: int = 0, flags: int = 0, host_threads: int = 0):
        opts = Opts()
        opts.host_chunk_packets = host_chunk_packets
        opts.flags = flags
        opts.host_threads = host_threads
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p(0)
        _check(lib().bt_group_create(devs, len(devices), ctypes.byref(opts), ctypes.byref(h)))
        self.h = h.value
        self.devices = list(devices)

    def close(self):
        if self.h:
            lib().bt_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return int(lib().bt_group_size(self.h))

    def member(self, k: int) -> int:
        return lib().bt_group_member(self.h, k)

    def placement(self, k: int) -> dict:
        p = Placement()
        _check(lib().bt_context_placement(self.member(k), ctypes.byref(p)))
        return p.as_dict()

    def cost(self, mapped: bool, records: bool, filters: bool, desc_bytes: int = 8):
        """bt_group_cost: the (window, align, fixed) model a call splits its batch by."""
        c = SplitCost()
        _check(lib().bt_group_cost(self.h, int(mapped), int(records), int(filters), desc_bytes, ctypes.byref(c)))
        return c.as_tuple()

    def register(self, arr: np.ndarray):
        """bt_group_host_register: page-lock + map a host array into every member's device."""
        _check(lib().bt_group_host_register(self.h, arr.ctypes.data, arr.nbytes))

    def unregister(self, arr: np.ndarray):
        _check(lib().bt_group_host_unregister(self.h, arr.ctypes.data))

    def run_mapped(self, batch: Batch, outs: Outputs):
        """bt_group_parse_filter_mapped: batch / outputs as host addresses in registered ranges."""
        _check(lib().bt_group_parse_filter_mapped(self.h, ctypes.byref(batch), ctypes.byref(outs)))

    def compile(self, filters):
        arr = filter_descs(filters)
        _check(lib().bt_group_filter_compile(self.h, arr, len(filters)))

    def run_host(self, data: np.ndarray, desc: np.ndarray, records=True, filters=True, outs: dict | None = None):
        """bt_group_parse_filter over host buffers (the same outputs as Context.run_host)."""
        return self._run(lambda *o: lib().bt_group_parse_filter(self.h, data.ctypes.data, desc.ctypes.data,
                                                                len(desc), *o),
                         len(desc), records, filters, keep=(np.ascontiguousarray(data),), outs=outs)

    def run_ptrs(self, frames, records=True, filters=True):
        """bt_group_parse_filter_ptrs over a list of frames (the std::vector<Packet> form)."""
        bufs = [np.frombuffer(bytes(f), np.uint8) if len(f) else np.zeros(1, np.uint8) for f in frames]
        ptrs = (ctypes.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
        lens = np.array([len(f) for f in frames], np.uint32)
        return self._run(lambda *o: lib().bt_group_parse_filter_ptrs(self.h, ptrs, lens.ctypes.data, len(frames), *o),
                         len(frames), records, filters, keep=(bufs, lens))

    def _run(self, call, n, records, filters, keep=(), outs=None):
        rec, ver, dec, pidx, npass = _host_outputs(n, records, filters, outs)
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        _check(call(p(rec), p(ver), p(dec), p(pidx), p(npass)))
        del keep
        out = {"records": rec, "verdict": ver, "decide": dec}
        if filters:
            out["pass_idx"] = pidx[: int(npass[0])]
            out["n_pass"] = int(npass[0])
        return out


def ring_walk_tpv3(ring: np.ndarray, block_size: int, n_blocks: int, first: int = 0,
                   max_blocks: int | None = None, cap: int | None = None, ctx: "Context | None" = None,
                   out: np.ndarray | None = None):
    """bt_ring_walk_tpv3 over a TPACKET_V3 ring image / mmap'd ring held in `ring` (uint8).
    Returns (desc uint64[n], blocks taken); with `out` (contiguous uint64) the descriptors
    are written there and desc is a view of it. Host-only: ctx may be None (no GPU)."""
    L = lib()
    if ring.nbytes < block_size * n_blocks:
        raise ValueError("ring buffer smaller than block_size * n_blocks")
    if out is not None:
        if out.dtype != np.uint64 or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous uint64 array")
        cap = len(out) if cap is None else min(cap, len(out))
        desc = out
    else:
        if cap is None:
            cap = int(ring.nbytes // 96) + 1
        desc = np.empty(max(cap, 1), dtype=np.uint64)
    r = Tpv3Ring(ring.ctypes.data, block_size, n_blocks, 0)
    nd, nb = ctypes.c_uint32(), ctypes.c_uint32()
    _check(L.bt_ring_walk_tpv3(ctx.h if ctx else None, ctypes.byref(r), first,
                               n_blocks if max_blocks is None else max_blocks, desc.ctypes.data, cap,
                               ctypes.byref(nd), ctypes.byref(nb)))
    return desc[:nd.value], nb.value


PREFIX_SLOT = 128
BATCH_PREFIXES = 0x1
BATCH_LEAN = 0x2


def ring_gather_tpv3(ring: np.ndarray, block_size: int, n_blocks: int, slots: np.ndarray, out: np.ndarray,
                     first: int = 0, max_blocks: int | None = None, ctx: "Context | None" = None,
                     slot_base: int = 0, dense: bool = False, ring_out: np.ndarray | None = None,
                     lean: bool = False):
    """bt_ring_gather_tpv3: the walk of ring_walk_tpv3, plus every frame's header prefix
    copied into slots[(slot_base + i) * PREFIX_SLOT ...]; descriptors (written to
    out[slot_base:]) point into `slots`. dense=True: bt_ring_gather_dense_tpv3 (each block's
    prefixes back to back from its first slot; ring_out[slot_base:] gets the ring descriptors).
    lean=True: bt_ring_gather_lean_tpv3 (filter-only: each frame's bytes 12..43, packed after a
    16-B pad; run the batch with BATCH_PREFIXES | BATCH_LEAN). Returns (desc view, blocks taken)."""
    if slots.dtype != np.uint8 or not slots.flags.c_contiguous or out.dtype != np.uint64:
        raise ValueError("slots must be contiguous uint8, out uint64")
    if ring_out is not None and (not (dense or lean) or ring_out.dtype != np.uint64 or len(ring_out) < len(out)):
        raise ValueError("ring_out: uint64, as long as out, dense or lean gather only")
    cap = min(len(out) - slot_base, len(slots) // PREFIX_SLOT - slot_base)
    r = Tpv3Ring(ring.ctypes.data, block_size, n_blocks, 0)
    nd, nb = ctypes.c_uint32(), ctypes.c_uint32()
    args = (ctx.h if ctx else None, ctypes.byref(r), first, n_blocks if max_blocks is None else max_blocks,
            slots.ctypes.data + slot_base * PREFIX_SLOT, out.ctypes.data + 8 * slot_base)
    tail = (cap, ctypes.byref(nd), ctypes.byref(nb))
    if dense or lean:
        rd = None if ring_out is None else ring_out.ctypes.data + 8 * slot_base
        fn = lib().bt_ring_gather_lean_tpv3 if lean else lib().bt_ring_gather_dense_tpv3
        _check(fn(*args, rd, *tail))
    else:
        _check(lib().bt_ring_gather_tpv3(*args, *tail))
    return out[slot_base:slot_base + nd.value], nb.value


RING_RESUME_PAYLOAD = 0x1


def ring_stage_tpv3(ctx: "Context", ring: np.ndarray, block_size: int, n_blocks: int, desc: np.ndarray,
                    decide: np.ndarray, verdict: np.ndarray | None = None, slots: np.ndarray | None = None,
                    first: int = 0, count: int | None = None, batch_blocks: int = 0, gather: bool = False,
                    in_place_every: int = 0, in_place_blocks: int = 0, resume_payload: bool = False,
                    ring_desc: np.ndarray | None = None, want_host: bool = False):
    """bt_ring_stage_tpv3: blocks [first, first + count) of a registered ring through the
    context's filter, walk of each batch overlapping the kernels of the one before. desc /
    decide (/ verdict, slots) are host arrays registered with ctx (abi.host_array + register).
    Returns (frames, passed).
    resume_payload / ring_desc / want_host: bt_ring_stage_tpv3_ex. resume_payload=True is
    BT_RING_RESUME_PAYLOAD (gathered batches of a program with a GPU PAYLOAD slot are finished by
    the resume kernel; ring_desc: registered uint64 array as long as desc, for the frames' ring
    descriptors). want_host=True returns (frames, passed, n_host), n_host = the frames whose final
    code is still DECIDE_HOST."""
    cap = min(len(desc), len(decide))
    if verdict is not None and len(verdict) * 64 < cap:
        raise ValueError("verdict: need ceil(cap / 64) words")
    if slots is not None and slots.nbytes < cap * PREFIX_SLOT:
        raise ValueError("slots: need cap * PREFIX_SLOT bytes")
    if ring_desc is not None and (ring_desc.dtype != np.uint64 or len(ring_desc) < cap):
        raise ValueError("ring_desc: uint64, at least as long as desc")
    r = Tpv3Ring(ring.ctypes.data, block_size, n_blocks, 0)
    o = RingStageOpts(batch_blocks, 2 if gather == "adaptive" else int(bool(gather)), in_place_every, in_place_blocks)
    nd, npass, nhost = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    head = (ctx.h, ctypes.byref(r), first, n_blocks if count is None else count, ctypes.byref(o))
    tail = (None if slots is None else slots.ctypes.data, decide.ctypes.data,
            None if verdict is None else verdict.ctypes.data, cap, ctypes.byref(nd), ctypes.byref(npass))
    if not (resume_payload or ring_desc is not None or want_host):
        _check(lib().bt_ring_stage_tpv3(*head, desc.ctypes.data, *tail))
        return nd.value, npass.value
    _check(lib().bt_ring_stage_tpv3_ex(*head, RING_RESUME_PAYLOAD if resume_payload else 0, desc.ctypes.data,
                                       None if ring_desc is None else ring_desc.ctypes.data, *tail,
                                       ctypes.byref(nhost)))
    return (nd.value, npass.value, nhost.value) if want_host else (nd.value, npass.value)


def ring_walk_tpv3_gpu(ctx: "Context", ring: np.ndarray, ring_dev: int, block_size: int, n_blocks: int,
                       desc_dev: int, cap: int, first: int = 0, max_blocks: int | None = None,
                       bad_dev: int | None = None, stream=None):
    """bt_ring_walk_tpv3_gpu: the host reads the ready blocks' headers, a kernel walks
    their frame chains through ring_dev (the ring's registered alias) and writes the
    descriptors into desc_dev (device memory). Returns (descriptors, blocks taken); the
    descriptors are ready once the context stream (or `stream`) has run the walk."""
    r = Tpv3Ring(ring.ctypes.data, block_size, n_blocks, 0)
    nd, nb = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().bt_ring_walk_tpv3_gpu(ctx.h, ctypes.byref(r), ring_dev, first,
                                       n_blocks if max_blocks is None else max_blocks, desc_dev, cap,
                                       ctypes.byref(nd), ctypes.byref(nb), bad_dev, stream))
    return nd.value, nb.value


def ring_release_tpv3(ring: np.ndarray, block_size: int, n_blocks: int, first: int, count: int):
    r = Tpv3Ring(ring.ctypes.data, block_size, n_blocks, 0)
    _check(lib().bt_ring_release_tpv3(ctypes.byref(r), first, count))


def payload_dfa(expr: str, flags: int = 0):
    """bt_payload_dfa_compile: the DFA blob (bytes), None when the expression is outside
    the GPU subset (it stays on the host), or raises BtError if std::regex rejects it.
    flags (DFA_*): bt_payload_dfa_compile_ex with them; DFA_EXTENDED widens the subset."""
    L = lib()
    e = expr.encode("latin-1")
    size = ctypes.c_uint32()

    def compile_(buf, cap):
        if flags:
            return L.bt_payload_dfa_compile_ex(e, flags, buf, cap, ctypes.byref(size))
        return L.bt_payload_dfa_compile(e, buf, cap, ctypes.byref(size))

    rc = compile_(None, 0)
    if rc == 11:
        return None
    if rc:
        raise BtError(rc, f"bt_payload_dfa_compile({expr!r}) = {rc}")
    buf = ctypes.create_string_buffer(size.value)
    _check(compile_(buf, size.value))
    return buf.raw


def payload_dfa_search(blob: bytes, s: bytes) -> bool:
    return bool(lib().bt_payload_dfa_search(blob, s, len(s)))


def payload_dfa_eval(blob: bytes, frame) -> bool:
    """applyPayloadFilter(frame) for the compiled (non-empty) expression, on the host."""
    f = bytes(frame)
    return bool(lib().bt_payload_dfa_eval(blob, f, len(f)))


def untile_records(buf: np.ndarray, n: int, planes: bool = False, ctx: "Context | None" = None,
                   n_cap: int | None = None) -> np.ndarray:
    """bt_rec[n] (AoS) from the packed device record layout (include/beatrice_gpu.h),
    unpacked by bt_record_unpack."""
    out = np.zeros((n, BT_REC_BYTES), np.uint8)
    buf = np.ascontiguousarray(buf)
    _check(lib().bt_record_unpack(ctx.h if ctx is not None else None, buf.ctypes.data,
                                  n if n_cap is None else n_cap, n, int(planes), out.ctypes.data, None))
    return out


def record_slabs(rec: np.ndarray) -> np.ndarray:
    """Slabs the packed device form of each bt_rec occupies (bt_record_slabs)."""
    ok = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, BT_REC_BYTES)[:, 25].astype(np.int64)
    nd = 5 + ((ok & L_VLAN0) != 0) + ((ok & L_VLAN1) != 0) + \
        np.where(ok & L_IPV4, 5, np.where(ok & L_IPV6, 10, 0)) + \
        np.where(ok & L_TCP, 5, np.where(ok & (L_UDP | L_ICMP), 2, 0))
    return (nd + 3) // 4


def pack_records(rec: np.ndarray) -> np.ndarray:
    """numpy restatement of the kernel's packed record (parse_packet<true>; test helper):
    bt_rec[n] -> [n, 24] packed dwords, zero past each record's stored slabs."""
    r = np.ascontiguousarray(rec).view(np.uint8).reshape(-1, BT_REC_BYTES).view("<u4").astype(np.uint64)
    n = len(r)
    present, ok = r[:, 6] & 0xFF, (r[:, 6] >> 8) & 0xFF
    det = r[:, 22]
    ok4, ok6 = (ok & L_IPV4) != 0, (ok & L_IPV6) != 0
    c = np.zeros((n, 24), np.uint64)
    c[:, 0:4] = r[:, 0:4]
    c[:, 4] = present | (ok << 8) | ((det & 7) << 16) | (((det >> 8) & 0xFF) << 19) | (((det >> 16) & 7) << 27)
    ne = ((ok & L_VLAN0) != 0).astype(np.int64) + ((ok & L_VLAN1) != 0)
    x0 = (r[:, 5] & 0xFFFF) | (r[:, 4] & 0xFFFF0000)
    x1 = r[:, 5] >> 16
    v4 = np.stack([(r[:, 7] & 0xFF) | ((r[:, 7] >> 8) & 0xFF00) | ((r[:, 7] >> 8) & 0xFF0000) | ((r[:, 8] & 0xFF) << 24),
                   (r[:, 8] >> 16) | ((r[:, 9] & 0xFFFF) << 16), (r[:, 9] >> 16) | ((r[:, 10] & 0xFFFF) << 16),
                   r[:, 11], r[:, 12]], axis=1)
    l4 = r[:, 17:22]
    L = np.zeros((n, 15), np.uint64)
    L[ok4, 0:5] = v4[ok4]
    L[ok4, 5:10] = l4[ok4]
    L[ok6, 0:10] = r[ok6, 7:17]
    L[ok6, 10:15] = l4[ok6]
    for e in (0, 1, 2):
        m = ne == e
        if e >= 1:
            c[m, 5] = x0[m]
        if e == 2:
            c[m, 6] = x1[m]
        c[m, 5 + e:20 + e] = L[m]
    return c.astype(np.uint32)


def tile_packed(c: np.ndarray, nslab: np.ndarray, planes: bool = False, seed: int = 1) -> np.ndarray:
    """Test helper: packed records [n, 24] in the device layout (tiled, or plane-major
    with n_cap = n). Slabs a record does not store hold random bytes, as on the device."""
    n = len(c)
    nt = (n + 63) // 64
    rng = np.random.default_rng(seed)
    slabs = c.reshape(n, 6, 16 // 4).view(np.uint8).reshape(n, 6, 16).copy()
    keep = np.arange(6)[None, :] < nslab[:, None]
    if planes:   # whole-wave slabs, one slot per packet
        slabs[~keep] = rng.integers(0, 256, size=(int((~keep).sum()), 16), dtype=np.uint8)
        return np.ascontiguousarray(slabs.transpose(1, 0, 2)).reshape(-1)
    # tiled: slabs 0..1 at the packet's slot (zeros for a last tile's unused slots), slab
    # k >= 2 packed in packet order to the front of the tile's slab-k region
    t = rng.integers(0, 256, size=(nt, 6, 64, 16), dtype=np.uint8)
    t[:, 0:2] = 0
    for i in range(n):
        tt, lane = divmod(i, 64)
        t[tt, 0:2, lane] = slabs[i, 0:2]
    for tt in range(nt):
        idx = np.arange(tt * 64, min(n, tt * 64 + 64))
        for k in range(2, 6):
            sel = idx[nslab[idx] > k]
            t[tt, k, :len(sel)] = slabs[sel, k]
    return t.reshape(-1)


class DeviceRun:
    """Device-resident batch + outputs (the bench / parity path)."""

    def __init__(self, ctx: Context, data: np.ndarray | None, desc: np.ndarray | None, n: int, stride: int = 0,
                 records=True, decide=True, verdict=True, pass_idx=True, data_bytes: int | None = None):
        """data=None: the packet buffer (data_bytes long) is filled later with upload_data()."""
        self.ctx, self.n = ctx, n
        nbytes = int(data.nbytes) if data is not None else int(data_bytes)
        self.d_data = ctx.alloc((nbytes + 255) // 256 * 256 + 256)
        if data is not None:
            self.d_data.upload(data)
        self.d_desc = None
        if desc is not None:
            self.d_desc = ctx.alloc(max(8, desc.nbytes))
            self.d_desc.upload(np.ascontiguousarray(desc, dtype=np.uint64))
        self.batch = Batch(self.d_data.ptr, self.d_desc.ptr if self.d_desc else None, stride, n, nbytes)
        nt = (n + 63) // 64
        self.d_rec = ctx.alloc(max(16, nt * 64 * BT_REC_BYTES)) if records else None
        self.d_dec = ctx.alloc(max(16, n)) if decide else None
        self.d_ver = ctx.alloc(max(16, nt * 8)) if verdict else None
        self.d_pidx = ctx.alloc(max(16, n * 4)) if pass_idx else None
        self.d_npass = ctx.alloc(16) if pass_idx else None
        self.outs = Outputs(self.d_rec.ptr if self.d_rec else None, n,
                            self.d_ver.ptr if self.d_ver else None,
                            self.d_dec.ptr if self.d_dec else None,
                            self.d_pidx.ptr if self.d_pidx else None,
                            self.d_npass.ptr if self.d_npass else None)
        ctx.reserve(n)
        self.alt, self.alt_outs = None, None

    def upload_data(self, buf: np.ndarray, offset: int):
        """Bytes of the packet buffer from `offset` on (a capture streamed range by range)."""
        self.d_data.upload(buf, offset)

    def run(self):
        self.ctx.run_device(self.batch, self.outs)

    def fetch(self):
        n = self.n
        out = {}
        self.ctx.synchronize()
        if self.d_rec:
            buf = self.d_rec.download(np.zeros(self.d_rec.nbytes, np.uint8))
            if self.ctx.flags & OPT_RECORDS_AOS:   # bt_rec as is
                out["records"] = buf[: n * BT_REC_BYTES].reshape(n, BT_REC_BYTES)
            else:
                out["records"] = untile_records(buf, n, planes=bool(self.ctx.flags & OPT_RECORDS_PLANES))
        if self.d_dec:
            out["decide"] = self.d_dec.download(np.zeros(n, dtype=np.uint8))
        if self.d_ver:
            out["verdict"] = self.d_ver.download(np.zeros((n + 63) // 64, dtype=np.uint64))
        if self.d_pidx:
            npass = int(self.d_npass.download(np.zeros(1, dtype=np.uint32))[0])
            out["n_pass"] = npass
            out["pass_idx"] = self.d_pidx.download(np.zeros(max(npass, 1), dtype=np.uint32))[:npass]
        return out

    def record_slabs(self) -> int:
        """Total 16-B slabs the last run stored (packed records), counted on the host."""
        if not self.d_rec:
            return 0
        if not hasattr(lib(), "bt_record_unpack"):   # A/B against a build from before packed records
            return 6 * self.n
        self.ctx.synchronize()
        buf = self.d_rec.download(np.zeros(self.d_rec.nbytes, np.uint8))
        if self.ctx.flags & OPT_RECORDS_AOS:   # bt_rec as is: what the packed form would need
            return int(record_slabs(buf[: self.n * BT_REC_BYTES].reshape(self.n, BT_REC_BYTES)).sum())
        tot = ctypes.c_uint64(0)
        _check(lib().bt_record_unpack(self.ctx.h, buf.ctypes.data, self.n, self.n,
                                      int(bool(self.ctx.flags & OPT_RECORDS_PLANES)), None, ctypes.byref(tot)))
        return int(tot.value)

    def n_pass(self) -> int:
        self.ctx.synchronize()
        return int(self.d_npass.download(np.zeros(1, dtype=np.uint32))[0]) if self.d_npass else 0

    def second_outputs(self) -> Outputs:
        """A second output set of the same shape (records, decide, verdict, pass_idx,
        n_pass as this run has them), for pipelined steps that alternate two sets."""
        if self.alt is None:
            self.alt = [self.ctx.alloc(b.nbytes) if b is not None else None
                        for b in (self.d_rec, self.d_ver, self.d_dec, self.d_pidx, self.d_npass)]
            r, v, d, p, c = (b.ptr if b is not None else None for b in self.alt)
            self.alt_outs = Outputs(r, self.n, v, d, p, c)
        return self.alt_outs

    def free(self):
        for b in (self.d_data, self.d_desc, self.d_rec, self.d_dec, self.d_ver, self.d_pidx, self.d_npass,
                  *(self.alt or [])):
            if b is not None:
                b.free()


class DeviceExtract:
    """Device-resident batch for bt_extract_device (user protocol tables)."""

    def __init__(self, ctx: Context, data: np.ndarray | None, desc: np.ndarray | None, n: int, fields, stride: int = 0,
                 desc_format: int = DESC_PACKED, image=True, batch: Batch | None = None):
        """data / desc are uploaded; or `batch` names packets already on the device
        (e.g. a DeviceRun's), which this object then neither owns nor frees."""
        self.ctx, self.n = ctx, n
        self.fields = list(fields)
        self.span = proto_span(self.fields)
        self.d_data = self.d_desc = None
        if batch is not None:
            self.batch = batch
        else:
            self.d_data = ctx.alloc((data.nbytes + 255) // 256 * 256 + 256)
            self.d_data.upload(data)
            if desc is not None:
                self.d_desc = ctx.alloc(max(16, desc.nbytes))
                self.d_desc.upload(np.ascontiguousarray(desc))
            self.batch = Batch(self.d_data.ptr, self.d_desc.ptr if self.d_desc else None, stride, n,
                               int(data.nbytes), desc_format, 0)
        nf = len(self.fields)
        img = image and 0 < self.span <= 0xFFFF
        self.d_status = ctx.alloc(max(16, n))
        self.d_values = ctx.alloc(max(16, nf * n * 8)) if nf else None
        self.d_image = ctx.alloc(max(16, n * self.span)) if img else None
        self.out = ExtractOut(self.d_status.ptr, self.d_values.ptr if self.d_values else None,
                              self.d_image.ptr if self.d_image else None, n, 0)
        self.table, self.nf = field_table(self.fields)

    def run(self, stream=None):
        _check(lib().bt_extract_device(self.ctx.h, ctypes.byref(self.batch), self.table, self.nf,
                                       ctypes.byref(self.out), stream))

    def time(self, iters: int, mode: int = TIME_KERNEL_EVENTS) -> Timing:
        """bt_time_extract2: `iters` launches; with TIME_KERNEL_EVENTS each is timed from
        its own dispatch (main_ms), without them only the span is."""
        t = Timing()
        _check(lib().bt_time_extract2(self.ctx.h, ctypes.byref(self.batch), self.table, self.nf,
                                      ctypes.byref(self.out), iters, mode, ctypes.byref(t)))
        return t

    def fetch(self):
        self.ctx.synchronize()
        n, nf = self.n, len(self.fields)
        status = self.d_status.download(np.zeros(max(n, 1), np.uint8))[:n]
        values = self.d_values.download(np.zeros(max(1, nf * n), np.uint64))[:nf * n].reshape(nf, n) \
            if self.d_values else np.zeros((nf, n), np.uint64)
        image = self.d_image.download(np.zeros(max(16, n * self.span), np.uint8))[:n * self.span].reshape(n, self.span) \
            if self.d_image else None
        return status, values, image

    def free(self):
        for b in (self.d_data, self.d_desc, self.d_status, self.d_values, self.d_image):
            if b is not None:
                b.free()

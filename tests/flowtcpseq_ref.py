"""Restatement of bt_flow_tcpseq_* (include/beatrice_gpu.h, "per-flow TCP sequence classification")
as a plain loop over Python integers with a dict per (flow, direction), written from the header's
text. Nothing here calls the code under test."""
import numpy as np

import flow_ref as fr
import flowtab_ref as ftr

SENTINELS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB)   # UNSELECTED, NONE, OVERFLOW, EXPIRED
NONE, FIRST, IN_ORDER, GAP, OLD, OVERLAP = range(6)
OFF_NONE = -(1 << 63)
DIR_REC = np.dtype({"names": ["pos", "hi", "last_seq", "have", "seq_packets", "old_packets", "gap_packets", "overlap_packets",
                              "old_bytes", "gap_bytes", "reserved"],
                    "formats": ["<i8", "<i8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8"],
                    "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56], "itemsize": 64})
REC = np.dtype({"names": ["d"], "formats": [(DIR_REC, 2)], "offsets": [0], "itemsize": 128})
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
COUNTS = ("seq_packets", "old_packets", "gap_packets", "overlap_packets", "old_bytes", "gap_bytes")


def segment_of(frame: bytes):
    """(s, L) of a frame with a whole TCP header under the statistics table's BT_FSEEN_L4 rule, or
    None. `frame` holds the bytes the call may read (zeros where `bytes` cut it); its length is the
    descriptor's. L comes from the header fields alone."""
    n = len(frame)
    be16 = lambda o: (frame[o] << 8) | frame[o + 1]  # noqa: E731
    if n < 14:
        return None
    et, k = be16(12), 0
    while k < 2 and et in (0x8100, 0x88A8):
        if n < 18 + 4 * k:
            return None
        et = be16(16 + 4 * k)
        k += 1
    o3 = 14 + 4 * k
    if et == 0x0800 and n - o3 >= 20:
        ihl = frame[o3] & 0xF
        o4, proto, ip_payload = o3 + 4 * ihl, frame[o3 + 9], be16(o3 + 2) - 4 * ihl
        if be16(o3 + 6) & 0x3FFF:
            return None
    elif et == 0x86DD and n - o3 >= 40:
        o4, proto, ip_payload = o3 + 40, frame[o3 + 6], be16(o3 + 4)
    else:
        return None
    if proto != 6 or o4 > n or n - o4 < 20:
        return None
    plen = max(0, ip_payload - 4 * (frame[o4 + 12] >> 4))
    flags = frame[o4 + 13]
    return int.from_bytes(frame[o4 + 4:o4 + 8], "big"), plen + (flags >> 1 & 1) + (flags & 1)


def direction(frame: bytes, table_flags: int) -> int:
    if not table_flags & ftr.BIDIRECTIONAL:
        return 0
    key, klass = fr.walk(frame, bool(table_flags & ftr.L3_ONLY))
    return ftr.canonical(key, klass)[1]


def int32(x: int) -> int:
    x &= M32
    return x - (1 << 32) if x >= 1 << 31 else x


class Space:
    """The sequence spaces of a table of `cap` flows: every batch stepped through in order."""

    def __init__(self, cap: int, table_flags: int = 0, start=None):
        self.cap, self.flags = cap, table_flags
        self.state = {}   # (flow, dir) -> dict of Python ints
        if start is not None:
            for f in range(cap):
                for d in range(2):
                    r = start[f]["d"][d]
                    if any(int(r[name]) for name in DIR_REC.names):
                        self.state[(f, d)] = {name: int(r[name]) for name in DIR_REC.names}

    @property
    def table(self):
        t = np.zeros(self.cap, REC)
        for (f, d), st in self.state.items():
            for name in DIR_REC.names:
                v = st[name]
                if name in ("pos", "hi"):
                    t[f]["d"][d][name] = v
                else:
                    t[f]["d"][d][name] = v & (M64 if name.endswith("bytes") or name == "reserved" else M32)
        return t

    def step(self, f: int, d: int, s: int, L: int):
        """One participating packet: (class, u)."""
        st = self.state.setdefault((f, d), {name: 0 for name in DIR_REC.names})
        oldb = gapb = 0
        if not st["have"]:
            u, k = 0, FIRST
            st["hi"], st["have"] = L, 1
        else:
            u = st["pos"] + int32(s - st["last_seq"])
            e, hi = u + L, st["hi"]
            if u == hi:
                k = IN_ORDER
            elif u > hi:
                k, gapb = GAP, u - hi
            elif e <= hi:
                k, oldb = OLD, L
            else:
                k, oldb = OVERLAP, hi - u
            st["hi"] = max(hi, e)
        st["pos"], st["last_seq"] = u, s
        st["seq_packets"] += 1
        st["old_packets"] += k == OLD
        st["gap_packets"] += k == GAP
        st["overlap_packets"] += k == OVERLAP
        st["old_bytes"] += oldb
        st["gap_bytes"] += gapb
        return k, u, oldb, gapb

    def batch(self, frames, flow_id, select=None):
        """One call: frames (bytes each, what the call may read), one flow id each, select words or
        None. Returns (cls, off, out_select words, result dict); the state moves on."""
        n = len(frames)
        nw = (n + 63) // 64
        cls, off, out = np.zeros(n, np.uint8), np.full(n, OFF_NONE, np.int64), np.zeros(nw, np.uint64)
        r = dict(n=n, selected=0, seq_packets=0, first=0, in_order=0, gap=0, old=0, overlap=0, unkeyed=0, bad_ids=0, seq_bytes=0,
                 old_bytes=0, gap_bytes=0)
        names = {FIRST: "first", IN_ORDER: "in_order", GAP: "gap", OLD: "old", OVERLAP: "overlap"}
        for i in range(n):
            if select is not None and not (int(select[i >> 6]) >> (i & 63)) & 1:
                continue
            r["selected"] += 1
            keep = True
            f = int(flow_id[i])
            if f >= self.cap:
                r["unkeyed" if f in SENTINELS else "bad_ids"] += 1
            else:
                seg = segment_of(frames[i])
                if seg is not None and seg[1] > 0:
                    k, u, oldb, gapb = self.step(f, direction(frames[i], self.flags), seg[0], seg[1])
                    cls[i], off[i] = k, u
                    r["seq_packets"] += 1
                    r["seq_bytes"] += seg[1]
                    r["old_bytes"] += oldb
                    r["gap_bytes"] += gapb
                    r[names[k]] += 1
                    keep = k != OLD
            if keep:
                out[i >> 6] |= np.uint64(1 << (i & 63))
        return cls, off, out, r

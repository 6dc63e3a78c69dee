"""Restatement of bt_flow_reasm_* (include/beatrice_gpu.h, "per-flow TCP reassembly") as a plain loop
over Python integers with a dict per (flow, direction), written from the header's text: the rules
1. - 8. in their order. The matcher's step is flowstream_ref.Masks (the Shift-And step over the
blob's masks). Nothing here calls the code under test."""
import numpy as np

import flowstream_ref as sr

SENTINELS = sr.SENTINELS
OFF_NONE = -(1 << 63)
NEW_BASE = -(1 << 30)
REL_MAX = 0x7FFE0000
DIR_REC = np.dtype({"names": ["d", "next", "have", "stream_packets", "hit_packets", "holes", "dup_packets", "late_packets",
                              "dup_bytes", "hole_bytes", "late_bytes"],
                    "formats": ["<u8", "<i8", "<u4", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", "<u8", "<u8"],
                    "offsets": [0, 8, 16, 20, 24, 28, 32, 36, 40, 48, 56], "itemsize": 64})
REC = np.dtype({"names": ["d"], "formats": [(DIR_REC, 2)], "offsets": [0], "itemsize": 128})
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
RESULT = ("n", "selected", "unkeyed", "bad_ids", "stream_packets", "hit_packets", "new_hit_flows", "holes", "dup_packets",
          "late_packets", "far_packets", "stream_bytes")


def tcp_payload(frame: bytes):
    """(start, end, SYN) of a TCP segment's captured payload by the stream matcher's rule, or None: not
    TCP, no whole header, or no payload byte in the frame."""
    pl = sr.payload_of(frame)
    if pl is None:
        return None
    o3 = 14
    while frame[o3 - 2:o3] in (b"\x81\x00", b"\x88\xa8"):
        o3 += 4
    v6 = frame[o3] >> 4 == 6
    proto = frame[o3 + 6] if v6 else frame[o3 + 9]
    if proto != 6:
        return None
    o4 = o3 + (40 if v6 else 4 * (frame[o3] & 0xF))
    return pl[0], pl[1], frame[o4 + 13] >> 1 & 1


class Reasm:
    """The reassembly records of a table of `cap` flows under one pattern: every call in order."""

    def __init__(self, cap: int, blob, table_flags: int = 0, start=None):
        self.cap, self.flags, self.masks = cap, table_flags, sr.Masks(blob)
        self.state = {}
        if start is not None:
            for f in range(cap):
                for d in range(2):
                    r = start[f]["d"][d]
                    if any(int(r[name]) for name in DIR_REC.names):
                        self.state[(f, d)] = {name: int(r[name]) for name in DIR_REC.names}

    def rec(self, f, d):
        return self.state.setdefault((f, d), {name: 0 for name in DIR_REC.names})

    @property
    def table(self):
        t = np.zeros(self.cap, REC)
        for (f, d), st in self.state.items():
            for name in DIR_REC.names:
                v = st[name]
                t[f]["d"][d][name] = v if name == "next" else v & (M64 if name.endswith("bytes") or name == "d" else M32)
        return t

    def batch(self, frames, flow_id, off, select=None):
        """One call: frames (bytes each, what the call may read), one flow id and one tcpseq offset each,
        select words or None. Returns (hit words, rest words, result dict); the state moves on."""
        n = len(frames)
        nw = (n + 63) // 64
        hit, rest = np.zeros(nw, np.uint64), np.zeros(nw, np.uint64)
        r = {k: 0 for k in RESULT}
        r["n"] = n
        hits_before = {k: st["hit_packets"] for k, st in self.state.items()}
        streams = {}
        for i in range(n):
            if select is not None and not (int(select[i >> 6]) >> (i & 63)) & 1:
                continue
            r["selected"] += 1
            if int(off[i]) == OFF_NONE:
                rest[i >> 6] |= np.uint64(1 << (i & 63))
            f = int(flow_id[i])
            if f >= self.cap:
                r["unkeyed" if f in SENTINELS else "bad_ids"] += 1
                continue
            if int(off[i]) == OFF_NONE:
                continue
            pl = tcp_payload(frames[i])
            if pl is None:
                continue
            start, end, syn = pl
            d = sr.direction(frames[i], self.flags)
            st = self.rec(f, d)
            ds = int(off[i]) + syn
            de = ds + (end - start)
            if st["have"]:
                nxt = st["next"]
                if de <= nxt:                       # 2.
                    st["late_packets"] += 1
                    st["late_bytes"] += end - start
                    r["late_packets"] += 1
                    continue
                base, trim = nxt, max(0, nxt - ds)   # 1., 3.
            else:
                base, trim = NEW_BASE, 0
            rel = ds + trim - base                  # 4.
            if rel < 0 or rel > REL_MAX:
                r["far_packets"] += 1
                continue
            st["dup_bytes"] += trim
            streams.setdefault((f, d), []).append((rel, i, bytes(frames[i][start + trim:end])))
        hit_flows = set()
        for (f, d), segs in streams.items():
            st = self.rec(f, d)
            segs.sort(key=lambda s: (s[0], s[1]))   # 5.
            D = st["d"] if st["have"] else 0
            hi = 0 if st["have"] else segs[0][0]
            for rel, i, data in segs:               # 6.
                if rel > hi:
                    st["holes"] += 1
                    st["hole_bytes"] += rel - hi
                    r["holes"] += 1
                    D = 0
                if rel + len(data) <= hi:
                    st["dup_packets"] += 1
                    st["dup_bytes"] += len(data)
                    r["dup_packets"] += 1
                    continue
                skip = max(hi - rel, 0)
                st["dup_bytes"] += skip
                D, got = self.masks.run(D, data[skip:])
                st["stream_packets"] += 1
                r["stream_packets"] += 1
                r["stream_bytes"] += len(data) - skip
                if got:
                    st["hit_packets"] += 1
                    r["hit_packets"] += 1
                    hit[i >> 6] |= np.uint64(1 << (i & 63))
                    hit_flows.add(f)
                hi = max(hi, rel + len(data))
            st["next"] = (st["next"] if st["have"] else NEW_BASE) + hi   # 7.
            st["have"], st["d"] = 1, D
        r["new_hit_flows"] = sum(1 for f in hit_flows if not hits_before.get((f, 0), 0) and not hits_before.get((f, 1), 0))
        return hit, rest, r

"""Restatement of bt_flow_stream_* (include/beatrice_gpu.h, "per-flow stream matching") as a plain
loop: the stream of (flow, direction) is a Python `bytes`, a packet is hit iff some match of the
pattern, by Python's `re`, ends at one of its stream bytes. Only the matcher's carried state d is
restated by the Shift-And step over the masks of the compiled blob, because `re` has no such state.
Nothing here calls the code under test."""
import re

import numpy as np

import flow_ref as fr
import flowtab_ref as ftr

SENTINELS = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB)   # UNSELECTED, NONE, OVERFLOW, EXPIRED
STREAM_REC = np.dtype({"names": ["d", "hit_packets", "stream_packets"], "formats": [("<u8", 2), ("<u4", 2), ("<u4", 2)],
                       "offsets": [0, 16, 24], "itemsize": 32})
M64 = (1 << 64) - 1


def payload_of(frame: bytes):
    """(start, end) of the L4 payload inside the frame, or None: a whole TCP / UDP header under the
    flow key's rule, the end at min(frame length, what the IP header says). `frame` holds the bytes
    the call may read (zeros where `bytes` cut it); its length is the descriptor's."""
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
        o4, proto, end3 = o3 + 4 * (frame[o3] & 0xF), frame[o3 + 9], o3 + be16(o3 + 2)
        if be16(o3 + 6) & 0x3FFF:
            return None
    elif et == 0x86DD and n - o3 >= 40:
        o4, proto, end3 = o3 + 40, frame[o3 + 6], o3 + 40 + be16(o3 + 4)
    else:
        return None
    need = {6: 20, 17: 8}.get(proto, 0)
    if not need or o4 > n or n - o4 < need:
        return None
    start = o4 + (4 * (frame[o4 + 12] >> 4) if proto == 6 else 8)
    end = min(n, end3)
    return (start, end) if end > start else None


def direction(frame: bytes, table_flags: int) -> int:
    if not table_flags & ftr.BIDIRECTIONAL:
        return 0
    key, klass = fr.walk(frame, bool(table_flags & ftr.L3_ONLY))
    return ftr.canonical(key, klass)[1]


class Masks:
    """The masks of a bit-parallel blob (bt_regex_dfa.cpp's layout), read from its bytes."""

    def __init__(self, blob):
        b = bytes(np.asarray(blob, np.uint8))
        assert b[0:2] == b"\xff\xff" and b[6] == 1 and int.from_bytes(b[8:12], "little") == 0
        self.W = int.from_bytes(b[2:4], "little")
        self.R = b[7]
        m = [int.from_bytes(b[16 + 8 * k:24 + 8 * k], "little") for k in range(7)]
        self.Iall, self.A, self.F = m[0], m[3], m[5]
        e = self.W // 8
        self.B = [int.from_bytes(b[80 + e * c:80 + e * (c + 1)], "little") for c in range(256)]
        every = 0
        for x in self.B:
            every |= x
        self.P = every.bit_length()

    def step(self, D: int, c: int) -> int:
        n = (((D << 1) & M64) | self.Iall) & self.B[c]
        for _ in range(self.R):
            n |= (n << 1) & self.A
        return n

    def run(self, D: int, data: bytes):
        """(the state after data, whether a match ended inside it), starting from state D."""
        hit = False
        for c in data:
            D = self.step(D, c)
            hit = hit or bool(D & self.F)
        return D, hit


class Streams:
    """The streams of a table of `cap` flows under one pattern: every batch appended in order."""

    def __init__(self, cap: int, py_pattern: str, blob, table_flags: int = 0, start=None):
        self.rx = re.compile(py_pattern.encode("latin-1"), re.DOTALL)
        self.masks = Masks(blob)
        self.P = self.masks.P
        self.flags = table_flags
        self.table = np.zeros(cap, STREAM_REC) if start is None else start.copy()
        self.by_masks = start is not None   # a starting state has no history for `re` to look at
        self.hist = {}
        self._memo = {}

    def _hit(self, stream: bytes, a: int, b: int) -> bool:
        lo = max(0, a - self.P)
        key = (stream[lo:b], a - lo)
        got = self._memo.get(key)
        if got is None:
            got = False
            for e in range(a + 1, b + 1):
                for s in range(max(0, e - self.P), e):
                    if self.rx.fullmatch(stream, s, e):
                        got = True
                        break
                if got:
                    break
            self._memo[key] = got
        return got

    def batch(self, frames, flow_id, select=None):
        """One call: frames (bytes each, what the call may read), one flow id each, select words or
        None. Returns (hit words, result dict); self.table moves on."""
        n, cap = len(frames), len(self.table)
        nw = (n + 63) // 64
        hit = np.zeros(nw, np.uint64)
        r = dict(n=n, selected=0, stream_packets=0, hit_packets=0, unkeyed=0, bad_ids=0, stream_bytes=0, new_hit_flows=0)
        before = self.table["hit_packets"].copy()
        hit_flows = set()
        for i in range(n):
            if select is not None and not (int(select[i >> 6]) >> (i & 63)) & 1:
                continue
            r["selected"] += 1
            f = int(flow_id[i])
            if f >= cap:
                r["unkeyed" if f in SENTINELS else "bad_ids"] += 1
                continue
            pl = payload_of(frames[i])
            if pl is None:
                continue
            d = direction(frames[i], self.flags)
            data = bytes(frames[i][pl[0]:pl[1]])
            old = self.hist.get((f, d), b"")
            new = old + data
            self.hist[(f, d)] = new
            rec = self.table[f]
            state, mask_hit = self.masks.run(int(rec["d"][d]), data)
            got = mask_hit if self.by_masks else self._hit(new, len(old), len(new))
            rec["d"][d] = state
            rec["stream_packets"][d] = (int(rec["stream_packets"][d]) + 1) & 0xFFFFFFFF
            r["stream_packets"] += 1
            r["stream_bytes"] += len(data)
            if got:
                rec["hit_packets"][d] = (int(rec["hit_packets"][d]) + 1) & 0xFFFFFFFF
                r["hit_packets"] += 1
                hit[i >> 6] |= np.uint64(1 << (i & 63))
                hit_flows.add(f)
        r["new_hit_flows"] = sum(1 for f in hit_flows if not before[f][0] and not before[f][1])
        return hit, r

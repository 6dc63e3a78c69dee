"""The case generator of the TCP reassembly tests, on flowtcpseq_cases.Conn and tcp. A conversation has a
true byte stream per direction; its segments are then swapped, delayed by several places, duplicated,
retransmitted with a different split, overlapped, dropped and spread over two or three calls. Every row
keeps what the generator knows: the true offset of its first data byte (`dstart`) and its bytes
(`data`); the named cases also say whether the packet must be hit (`hit`). The offsets the calls see come
from bt_flow_tcpseq_host on the same rows, never from here."""
import string

import numpy as np

import flowtcpseq_cases as tc
from flowtcpseq_cases import ACK, FIN, M32, PSH, SYN, Conn, Row, tcp

PATTERN = "HELLO"
LONG = (string.ascii_letters + string.digits)[:62] + "ab"   # 64 positions: T = 63


def seg(c, d, off, data, flags=ACK | PSH, hit=None, **kw):
    """The segment of connection c, direction d, whose sequence number is the true offset `off`, with
    the payload `data`."""
    r = c.seg(d, off, len(data), flags, payload=data, **kw)
    r.data, r.dstart, r.hit = bytes(data), off + bool(flags & SYN), hit
    return r


def other(frame, flow, hit=False):
    r = Row(frame, flow)
    r.data, r.dstart, r.hit = b"", 0, hit
    return r


def crafted():
    """The named cases under PATTERN, each in a flow of its own, over two calls: (calls, cap, expect).
    expect: {flow: {(direction, field): value}} of the records after the last call."""
    calls, expect = [[], []], {}
    f = 0

    def conn(isn0=1000, isn1=5000):
        nonlocal f
        c = Conn(f, isn0, isn1, sp=40000 + f)
        f += 1
        return c

    c = conn()   # 0: a pattern across two swapped segments
    calls[0] += [seg(c, 0, 6, b"LOdef", hit=True), seg(c, 0, 0, b"abcHEL", hit=False)]
    expect[c.flow] = {(0, "next"): 5, (0, "holes"): 0, (0, "hit_packets"): 1, (0, "stream_packets"): 2}
    c = conn()   # 1: three 1-byte segments in reverse order behind an in-order one
    calls[0] += [seg(c, 0, 0, b"xHE", hit=False), seg(c, 0, 5, b"O", hit=True), seg(c, 0, 4, b"L", hit=False), seg(c, 0, 3, b"L", hit=False)]
    c = conn()   # 2: a trim in the middle of a 128-byte piece of a 300-byte segment
    s = bytearray(b"." * 340)
    s[98:103] = b"HELLO"
    s[226:231] = b"HELLO"
    calls[0] += [seg(c, 0, 0, s[0:100], hit=False), seg(c, 0, 40, s[40:340], hit=True)]
    expect[c.flow] = {(0, "dup_bytes"): 60, (0, "hit_packets"): 1, (0, "next"): 340}
    c = conn()   # 3: a retransmit with different bytes: the first in (rel, index) order wins
    calls[0] += [seg(c, 0, 0, b"xxHEL", hit=False), seg(c, 0, 5, b"LOyy", hit=True), seg(c, 0, 5, b"XXyy", hit=False)]
    expect[c.flow] = {(0, "dup_packets"): 1, (0, "dup_bytes"): 4}
    c = conn()   # 4: ... and the other way round
    calls[0] += [seg(c, 0, 0, b"xxHEL", hit=False), seg(c, 0, 5, b"XXyy", hit=False), seg(c, 0, 5, b"LOyy", hit=False)]
    c = conn()   # 5: a hole inside a would-be match
    calls[0] += [seg(c, 0, 0, b"xxHEL", hit=False), seg(c, 0, 6, b"LOyy", hit=False)]
    expect[c.flow] = {(0, "holes"): 1, (0, "hole_bytes"): 1, (0, "hit_packets"): 0}
    c = conn()   # 6: a hole filled in the same call
    calls[0] += [seg(c, 0, 0, b"xHE", hit=False), seg(c, 0, 4, b"LOy", hit=True), seg(c, 0, 3, b"L", hit=False)]
    expect[c.flow] = {(0, "holes"): 0, (0, "hit_packets"): 1}
    c = conn()   # 7: a hole filled in the next call: late
    calls[0] += [seg(c, 0, 0, b"xHE", hit=False), seg(c, 0, 4, b"LOy", hit=False)]
    calls[1] += [seg(c, 0, 3, b"L", hit=False), seg(c, 0, 7, b"HELLO", hit=True)]
    expect[c.flow] = {(0, "holes"): 1, (0, "late_packets"): 1, (0, "late_bytes"): 1, (0, "hit_packets"): 1, (0, "next"): 12}
    c = conn()   # 8: a segment straddling next across calls
    calls[0] += [seg(c, 0, 0, b"xxHE", hit=False)]
    calls[1] += [seg(c, 0, 2, b"HELLOzz", hit=True)]
    expect[c.flow] = {(0, "dup_bytes"): 2, (0, "next"): 9}
    c = conn()   # 9: a SYN with data, and a FIN
    calls[0] += [seg(c, 0, 0, b"HEL", SYN, hit=False), seg(c, 0, 4, b"LO", FIN | ACK, hit=True), seg(c, 0, 7, b"", ACK)]
    expect[c.flow] = {(0, "next"): 6}
    c = conn(M32 + 1 - 3)   # 10: the 2^32 wrap inside a match, in reverse arrival
    calls[0] += [seg(c, 0, 5, b"Oz", hit=True), seg(c, 0, 3, b"LL", hit=False), seg(c, 0, 0, b"qHE", hit=False)]
    c = conn()   # 11: a snapped frame: 10 of 100 payload bytes captured, the rest is a hole
    calls[0] += [seg(c, 0, 0, b"xxxxxxxHEL" + b"LO" * 45, snap=64, hit=False), seg(c, 0, 100, b"LOyy", hit=False)]
    expect[c.flow] = {(0, "holes"): 1, (0, "hole_bytes"): 90}
    c = conn()   # 12: a far segment
    calls[0] += [seg(c, 0, 0, b"HELLO", hit=True)]
    calls[1] += [seg(c, 0, 0x7FFF0000, b"HELLO", hit=False), seg(c, 0, 5, b"HELLO", hit=True)]
    expect[c.flow] = {(0, "next"): 10, (0, "stream_packets"): 2}
    c = conn()   # 13: both directions at once
    calls[0] += [seg(c, 0, 3, b"LO", hit=True), seg(c, 1, 3, b"LO", hit=True), seg(c, 1, 0, b"HEL", hit=False), seg(c, 0, 0, b"HEL", hit=False)]
    c = conn()   # 14: what is not placed goes to rest; sentinels and bad ids
    calls[0] += [seg(c, 0, 0, b"HEL", hit=False), other(tcp(1, payload=b"HELLO", proto=17, sp=40000 + c.flow), c.flow),
                 other(bytes(12) + b"\x08\x06" + bytes(50), c.flow), seg(c, 0, 3, b"", ACK), seg(c, 0, 3, b"LO", hit=True)]
    cap = f
    for sid in tc.SENTINEL_IDS:
        calls[1].append(other(tcp(1, payload=b"HELLO"), sid))
    calls[1] += [other(tcp(1, payload=b"HELLO"), cap), other(tcp(1, payload=b"HELLO"), 0x7FFFFFFF)]
    unsel = seg(Conn(0, 1000, 5000, sp=40000), 0, 11, b"HELLO", hit=False)
    unsel.sel = False
    calls[1].append(unsel)
    return calls, cap, expect


def long_pattern():
    """LONG (64 positions) across tiny segments in reverse arrival: (calls, cap)."""
    c = Conn(0, 77, 99)
    s = b"__" + LONG.encode() + b"__" + LONG.encode()[:63] + b"!"
    rows, at = [], 0
    for ln in [3, 7, 11, 2, 1, 13, 17, 5, 1, 1, 4, 9, 6, 19, 8, 3, 2, 16, 1, 4]:
        if at < len(s):
            rows.append(seg(c, 0, at, s[at:at + ln]))
            at += ln
    assert at >= len(s)
    return [rows[::-1]], 1


def conversation(rng, flow, nbytes, ncalls, clean, text=PATTERN.encode()):
    """One connection with both directions: per direction a true stream with `text` planted, cut into
    segments and spread over ncalls calls, then disturbed inside each call. With clean, nothing is
    dropped and nothing crosses a call: no hole, no late segment. Returns ([rows per call], {(flow, d):
    stream})."""
    c = Conn(flow, M32 + 1 - int(rng.integers(1, 60)) if flow == 0 else int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)),
             sp=42000 + flow % 20000)
    calls, truth = [[] for _ in range(ncalls)], {}
    for d in range(2):
        s = bytearray(rng.choice(np.frombuffer(b"HELO.", np.uint8), nbytes).tobytes())
        for at in rng.integers(0, max(1, nbytes - len(text)), max(1, nbytes // 40)):
            s[at:at + len(text)] = text
        truth[(flow, d)] = bytes(s)
        segs, at = [], 0
        while at < nbytes:
            ln = int(rng.choice([1, 2, 3, 7, 20, 60, 150, 300]))
            segs.append((at, min(nbytes, at + ln)))
            at += ln
        cuts = sorted(int(x) for x in rng.integers(0, len(segs) + 1, ncalls - 1))
        parts = [segs[a:b] for a, b in zip([0] + cuts, cuts + [len(segs)])]
        for k, part in enumerate(parts):
            rows = [seg(c, d, 0, b"", SYN)] if k == 0 else []
            rows += [seg(c, d, 1 + a, s[a:b]) for a, b in part]
            out = []
            for j, r in enumerate(rows):
                op = int(rng.integers(0, 12))
                out.append(r)
                if not r.data:
                    continue
                if op == 0 and len(out) > 1:                      # swapped with the one before
                    out[-1], out[-2] = out[-2], out[-1]
                elif op == 1:                                     # delayed by several places
                    out.insert(max(0, len(out) - 1 - int(rng.integers(2, 6))), out.pop())
                elif op == 2:                                     # duplicated, at once or later
                    out.insert(int(rng.integers(0, len(out) + 1)), r.again_data())
                elif op == 3 and j + 1 < len(rows) and j:         # retransmitted with a different split
                    a = rows[j].dstart - 1 - min(2, len(rows[j - 1].data))
                    out.append(seg(c, d, 1 + a, s[a:rows[j].dstart - 1 + len(r.data) // 2 + 1]))
                elif op == 4 and j:                               # an overlap from inside the one before
                    a = rows[j].dstart - 1 - (len(rows[j - 1].data) + 1) // 2
                    out.append(seg(c, d, 1 + a, s[a:rows[j].dstart - 1 + len(r.data)]))
                elif op == 5 and not clean:                       # dropped
                    out.pop()
                elif op == 6 and not clean and k + 1 < ncalls:    # arrives a call late
                    calls[k + 1].append(out.pop())
            calls[k] = tc.merge([calls[k], out], rng)
    return calls, truth


def again_data(self):
    r = self.again()
    r.data, r.dstart, r.hit = self.data, self.dstart, None
    return r


Row.again_data = again_data


def random_calls(seed, nflows=3, nbytes=600, ncalls=3, clean=True):
    """nflows conversations merged call by call into one arrival order: ([rows per call], truth)."""
    rng = np.random.default_rng(seed)
    per, truth = [[] for _ in range(ncalls)], {}
    for f in range(nflows):
        calls, t = conversation(rng, f, nbytes, ncalls, clean)
        truth.update(t)
        for k in range(ncalls):
            per[k].append(calls[k])
    return [tc.merge(streams, rng) for streams in per], truth


def in_order(nflows=3, nbytes=400, seed=1):
    """Every stream in order, no duplicates, with UDP packets of the same flows in between: one call."""
    rng = np.random.default_rng(seed)
    streams = []
    for f in range(nflows):
        c = Conn(f, int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), sp=43000 + f)
        for d in range(2):
            s = bytearray(rng.choice(np.frombuffer(b"HELO.", np.uint8), nbytes).tobytes())
            for at in range(17, nbytes - 5, 61):
                s[at:at + 5] = PATTERN.encode()
            rows, at = [], 0
            while at < nbytes:
                ln = int(rng.choice([1, 2, 5, 30, 200]))
                rows.append(seg(c, d, at, s[at:at + ln]))
                if ln == 5:
                    rows.append(other(tcp(1, payload=s[at:at + 9], proto=17, rev=bool(d), sp=43000 + f), f, hit=None))
                at += ln
            streams.append(rows)
    return [tc.merge(streams, rng)]

"""The frame builder and the case generator of the TCP sequence classification tests. A conversation
is built from true 64-bit stream offsets and an ISN; its segments are then dropped, duplicated,
swapped and split. For every packet the generator records the class that follows from the true
offsets (`truth`), which never wrap: the restatement and the code under test see the 32-bit wire
numbers alone and must arrive at the same classes."""
import struct

import numpy as np

NONE, FIRST, IN_ORDER, GAP, OLD, OVERLAP = range(6)
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10
CLIENT, SERVER = (10, 1, 2, 3), (10, 3, 2, 1)   # CLIENT sorts first: its packets are direction 0 of a bidirectional table
M32 = (1 << 32) - 1
SENTINEL_IDS = (0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFB)


def tcp(seq, plen=0, flags=ACK, rev=False, sp=40000, dp=80, payload=None, proto=6, ihl=5, tcp_words=5, vlan=None, v6=False, pad=0,
        snap=None, frag=0, ack=1):
    """An Ethernet frame around one TCP segment with sequence number `seq` and `plen` payload bytes (or
    `payload`), from CLIENT to SERVER or, with rev, the other way; the variants of flowstream_cases.frame
    and `frag`, the IPv4 flags / fragment offset field."""
    body = bytes(payload) if payload is not None else bytes((seq + k) & 0xFF for k in range(plen))
    src, dst = (SERVER, CLIENT) if rev else (CLIENT, SERVER)
    if rev:
        sp, dp = dp, sp
    if proto == 17:
        seg = struct.pack(">HHHH", sp, dp, 8 + len(body), 0) + body
    else:
        seg = struct.pack(">HHIIBBHHH", sp, dp, seq & M32, ack, tcp_words << 4, flags, 1024, 0, 0) + bytes(4 * (tcp_words - 5)) + body
    if v6:
        ip = struct.pack(">IHBB", 6 << 28, len(seg), proto, 64) + bytes(12) + bytes(src) + bytes(12) + bytes(dst)
    else:
        ip = struct.pack(">BBHHHBBH", 0x40 | ihl, 0, 4 * ihl + len(seg), 0, frag, 64, proto, 0) + bytes(src) + bytes(dst) + bytes(4 * (ihl - 5))
    eth = bytes(12) + (b"\x81\x00" + struct.pack(">H", vlan) if vlan is not None else b"") + (b"\x86\xdd" if v6 else b"\x08\x00")
    f = eth + ip + seg + bytes(pad)
    return f if snap is None else f[:snap]


class Row:
    """One packet of a case: its frame, flow id, select bit, and what the generator knows: the (flow,
    direction) it belongs to with its true offset and sequence length, or key None for a packet that
    does not participate."""

    def __init__(self, frame, flow, sel=True, key=None, off=0, L=0, batch=0):
        self.frame, self.flow, self.sel, self.key, self.off, self.L, self.batch = frame, flow, sel, key, off, L, batch
        self.want = NONE   # filled in by truth()

    def again(self):
        """The same packet once more: a row of its own, so that truth() can tell the two apart."""
        return Row(self.frame, self.flow, self.sel, self.key, self.off, self.L, self.batch)


class Conn:
    """One connection: flow number, a source port and an ISN per direction. seg() makes the packet of
    true offset `off` (0 = the SYN) in direction d."""

    def __init__(self, flow, isn0, isn1=7, sp=40000):
        self.flow, self.isn, self.sp = flow, (isn0, isn1), sp

    def seg(self, d, off, plen, flags=ACK | PSH, sel=True, **kw):
        L = plen + bool(flags & SYN) + bool(flags & FIN)
        f = tcp(self.isn[d] + off, plen, flags, rev=bool(d), sp=self.sp, **kw)
        return Row(f, self.flow, sel, (self.flow, d) if L else None, off, L)

    def ack(self, d, off, flags=ACK):
        """A pure ACK, or with RST a zero-length reset: it does not participate."""
        return Row(tcp(self.isn[d] + off, 0, flags, rev=bool(d), sp=self.sp), self.flow)

    def stream(self, d, lens, syn=True, fin=True, start=0):
        """The in-order segments of a direction from true offset `start`: SYN, data of `lens`, FIN."""
        rows, off = [], start
        if syn:
            rows.append(self.seg(d, off, 0, SYN))
            off += 1
        for ln in lens:
            rows.append(self.seg(d, off, ln))
            off += ln
        if fin:
            rows.append(self.seg(d, off, 0, FIN | ACK))
        return rows


def truth(rows):
    """The class of every row, in order, from the true offsets: per (flow, direction) the highest true
    end seen. Also the unwrapped start the call must report: the true offset less the direction's
    first. Rows that are unselected, carry no key or a flow that is no flow number are NONE."""
    hi, origin = {}, {}
    for r in rows:
        r.want, r.u = NONE, None
        if not r.sel or r.key is None or r.flow in SENTINEL_IDS or r.flow != r.key[0]:
            continue
        k = r.key
        if k not in hi:
            origin[k], hi[k], r.want = r.off, r.off + r.L, FIRST
        else:
            e = r.off + r.L
            r.want = IN_ORDER if r.off == hi[k] else GAP if r.off > hi[k] else OLD if e <= hi[k] else OVERLAP
            hi[k] = max(hi[k], e)
        r.u = r.off - origin[k]
    return rows


def disturb(rows, rng, rate=0.25):
    """A direction's in-order rows with some dropped, duplicated (at once or two places later), swapped
    with their neighbour, or followed by a retransmit that starts inside them and ends past them."""
    out, k = [], 0
    rows = list(rows)
    while k < len(rows):
        r = rows[k]
        op = rng.integers(0, 5) if rng.random() < rate and k else -1
        if op == 0:
            pass   # lost
        elif op == 1:
            out += [r, r.again()]
        elif op == 2:
            out.append(r)
            rows.insert(min(len(rows), k + 3), r.again())
        elif op == 3 and k + 1 < len(rows):
            out += [rows[k + 1], r]
            k += 1
        else:
            out.append(r)
        k += 1
    return out


def merge(streams, rng):
    """The streams' rows in one arrival order: each stream keeps its own."""
    left = [list(s) for s in streams if s]
    out = []
    while left:
        j = int(rng.integers(0, len(left)))
        out.append(left[j].pop(0))
        if not left[j]:
            left.pop(j)
    return out


def checked(rows):
    """What every case set must hold, from the generator alone: each of the five classes, an ISN within 100
    bytes of 2^32 (a wrap mid-stream), both directions in at least one flow."""
    truth(rows)
    got = {r.want for r in rows}
    assert got >= {FIRST, IN_ORDER, GAP, OLD, OVERLAP}, got
    keys = {r.key for r in rows if r.want != NONE}
    assert any((f, 0) in keys and (f, 1) in keys for f, _ in keys)
    wraps = False
    for k in keys:
        mine = [r for r in rows if r.key == k and r.want != NONE]
        first = int.from_bytes(tcp_seq_bytes(mine[0].frame), "big") - mine[0].off
        wraps = wraps or ((-first) & M32) <= 100 and max(r.off + r.L for r in mine) > ((-first) & M32)
    assert wraps
    return rows


def tcp_seq_bytes(frame):
    o3 = 14 + (4 if frame[12:14] == b"\x81\x00" else 0)
    o4 = o3 + (40 if frame[o3] >> 4 == 6 else 4 * (frame[o3] & 0xF))
    return frame[o4 + 4:o4 + 8]


def crafted():
    """The named cases over two batches and `cap` flows: (rows, cap)."""
    rows = []
    a = Conn(0, M32 + 1 - 50, 1000)                    # wraps after 50 bytes
    rows += a.stream(0, [20, 20, 20, 20], fin=False)   # SYN, data across the wrap
    rows.append(a.ack(1, 0))
    rows.append(a.seg(1, 0, 0, SYN | ACK))             # the other direction's first
    rows.append(a.seg(0, 0, 0, SYN))                   # a SYN retransmit: OLD
    rows.append(a.seg(0, 61, 20))                      # a retransmit: OLD
    rows.append(a.seg(0, 81, 20))                      # in order
    rows.append(a.seg(0, 121, 20))                     # 20 bytes lost: GAP
    rows.append(a.seg(0, 101, 20))                     # the hole filled late: OLD (no hole list)
    rows.append(a.seg(0, 131, 30))                     # OVERLAP: 10 old, 20 new
    rows.append(a.seg(0, 161, 0, FIN | ACK))           # FIN consumes one
    rows.append(a.seg(0, 161, 0, FIN | ACK))           # and its retransmit is OLD
    rows.append(a.seg(1, 1, 100))
    rows.append(a.ack(0, 162))
    rows.append(a.ack(1, 101, RST | ACK))              # a zero-length RST
    rows.append(a.seg(1, 101, 5, RST | ACK))           # RST adds nothing, its 5 bytes do
    b = Conn(1, 0x7FFFFFF0, M32 - 3, sp=40001)
    for kw in (dict(ihl=7), dict(vlan=5), dict(tcp_words=8), dict(pad=6), dict(v6=True)):   # each variant a flow of its own: in order, then old
        c = Conn(b.flow, b.isn[0], b.isn[1], sp=b.sp)
        rows += [c.seg(0, 0, 10, **kw), c.seg(0, 10, 10, **kw), c.seg(0, 0, 10, **kw), c.seg(1, 0, 9, **kw), c.seg(1, 9, 9, **kw)]
        b = Conn(b.flow + 1, b.isn[0] + 17, b.isn[1], sp=b.sp + 1)
    snapped = Conn(b.flow, 5, 5, sp=41000)             # snapped inside the payload: the header fields still advance
    rows += [snapped.seg(0, 0, 1000, snap=80), snapped.seg(0, 1000, 1000, snap=80), snapped.seg(0, 2500, 100, snap=80)]
    nots = Conn(b.flow + 1, 9, 9, sp=41001)            # what does not participate, between two in-order packets
    rows.append(nots.seg(0, 0, 10))
    rows += [Row(tcp(nots.isn[0] + 10, 10, proto=17, sp=41001), nots.flow),               # UDP
             Row(tcp(nots.isn[0] + 10, 10, frag=0x2000, sp=41001), nots.flow),            # MF set
             Row(tcp(nots.isn[0] + 10, 10, frag=0x0010, sp=41001), nots.flow),            # a fragment offset
             Row(tcp(nots.isn[0] + 10, 10, sp=41001)[:14 + 20 + 19], nots.flow),          # a truncated TCP header
             nots.ack(0, 10), nots.ack(0, 10, RST),
             nots.seg(0, 10, 10, sel=False)]                                              # unselected
    rows.append(nots.seg(0, 10, 10))
    half = Conn(b.flow + 2, 100, 100, sp=41002)        # a step of exactly 2^31 is taken as -2^31
    rows += [half.seg(0, 0, 10), half.seg(0, -(1 << 31), 10), half.seg(0, 10 - (1 << 31), 10), half.seg(0, 9, 10)]   # and back by 2^31 - 1
    cap = b.flow + 3
    for s in SENTINEL_IDS:
        rows.append(Row(tcp(1, 10), s, True, None))
    rows.append(Row(tcp(1, 10), cap))                  # a bad id
    rows.append(Row(tcp(1, 10), 0x7FFFFFFF))
    for r in rows[len(rows) // 2:]:
        r.batch = 1
    return checked(rows), cap


def random_set(seed, nflows=4, nseg=12, rate=0.3):
    """nflows connections with both directions, disturbed and merged into one arrival order; the first
    one's ISN lies 1 .. 100 below 2^32."""
    rng = np.random.default_rng(seed)
    streams, conns = [], []
    for f in range(nflows):
        c = Conn(f, M32 + 1 - int(rng.integers(1, 101)) if f == 0 else int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), sp=42000 + f)
        conns.append(c)
        for d in range(2):
            lens = [int(x) for x in rng.choice([1, 7, 100, 536, 1460], nseg)]
            s = disturb(c.stream(d, lens), rng, rate)
            for k in range(1, len(s), 4):
                s.insert(k, c.ack(d, 1))
            streams.append(s)
    rows = merge(streams, rng)
    # the classes a small set may miss by chance, planted behind the rest in flow 0, direction 0
    c0 = conns[0]
    end = max(r.off + r.L for r in rows if r.key == (0, 0))
    rows += [c0.seg(0, end + 100, 100), c0.seg(0, end + 150, 100), c0.seg(0, end + 250, 50), c0.seg(0, end + 250, 50)]   # GAP, OVERLAP, IN_ORDER, OLD
    return checked(rows)


def batches_of(rows):
    """[(frames, ids, select bit list, rows)] per batch."""
    out = []
    for b in sorted({r.batch for r in rows}):
        mine = [r for r in rows if r.batch == b]
        out.append(([r.frame for r in mine], [r.flow for r in mine], [r.sel for r in mine], mine))
    return out


def one_direction(n, dup_at=(), flow=0, isn=M32 - 40, plen=3, d=0):
    """n in-order segments of one (flow, direction), the ones at the list positions dup_at repeating the
    segment before them: rows with truth."""
    c = Conn(flow, isn, isn)
    rows, off = [], 0
    for k in range(n):
        if k in dup_at and k:
            rows.append(c.seg(d, off - plen, plen))
        else:
            rows.append(c.seg(d, off, plen))
            off += plen
    return rows

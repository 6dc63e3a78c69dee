"""The patterns and the frame builders of the stream matching tests. A pattern is spelled once: only
constructs on which ECMAScript (std::regex, the compiler's acceptance) and Python's `re` agree are
used: literals, bracket classes, \\d, \\x.., ?, | and (?:...); no `.` and no `$`."""
import struct

# (pattern, its positions P, a text that matches it): widths on both sides of every table entry
# width (8 / 16 / 32 / 64 bits), optional positions, a binary signature, a distributed group
PATTERNS = [
    ("GET|POST", 7, b"POST"),
    ("HTTP/1\\.[01]", 8, b"HTTP/1.1"),
    ("PUT|DELETE", 9, b"DELETE"),
    ("POST /index\\.html", 16, b"POST /index.html"),
    ("Host: example\\.com", 17, b"Host: example.com"),
    ("User-Agent: Mozilla/5\\.0 \\(X11; Li", 32, b"User-Agent: Mozilla/5.0 (X11; Li"),
    ("User-Agent: Mozilla/5\\.0 \\(X11; Lin", 33, b"User-Agent: Mozilla/5.0 (X11; Lin"),
    ("0123456789abcdef|ghijklmnopqrstuv|wxyzABCDEFGHIJKL|MNOPQRSTUVWXYZ-_", 64, b"wxyzABCDEFGHIJKL"),
    ("colou?r", 6, b"color"),
    ("ab?c?d\\d", 5, b"ad7"),
    ("\\x16\\x03[\\x00-\\x03]", 3, b"\x16\x03\x01"),
    ("(?:GET|HEAD) /x", 13, b"HEAD /x"),
    ("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789?-_", 64,
     b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ012345678-_"),
]

# what bt_flow_stream_compile refuses, one per construct: (pattern, a word of the message)
REFUSED = [
    ("GET.+", "repeatable"), ("ab*c", "repeatable"), ("a{2,}b", "repeatable"), ("^GET", "^"), ("done$", "$"),
    ("\\bGET", "subset"), ("(?:ab)+c", "DFA"), ("a?", "always"), ("a^b", "never"),
]
NOT_A_REGEX = ["(", "[a-"]

CLIENT, SERVER = (10, 1, 2, 3), (10, 3, 2, 1)


def _l4(proto, sp, dp, payload, tcp_words=5):
    if proto == 17:
        return struct.pack(">HHHH", sp, dp, 8 + len(payload), 0) + payload
    return struct.pack(">HHIIBBHHH", sp, dp, 1, 1, tcp_words << 4, 0x18, 1024, 0, 0) + bytes(4 * (tcp_words - 5)) + payload


def frame(payload=b"", src=CLIENT, dst=SERVER, sp=40000, dp=80, proto=6, ihl=5, tcp_words=5, vlan=None, v6=False, pad=0, snap=None):
    """An Ethernet frame around `payload`: IPv4 (ihl words) or IPv6, TCP (tcp_words) or UDP, one VLAN tag
    if vlan is a number; `pad` bytes of Ethernet padding behind the IP packet; cut to `snap` bytes."""
    seg = _l4(proto, sp, dp, bytes(payload), tcp_words)
    if v6:
        a, b = bytes(12) + bytes(src), bytes(12) + bytes(dst)
        ip = struct.pack(">IHBB", 6 << 28, len(seg), proto, 64) + a + b
    else:
        ip = struct.pack(">BBHHHBBH", 0x40 | ihl, 0, 4 * ihl + len(seg), 0, 0, 64, proto, 0) + bytes(src) + bytes(dst) + bytes(4 * (ihl - 5))
    eth = bytes(12) + (b"\x81\x00" + struct.pack(">H", vlan) if vlan is not None else b"") + (b"\x86\xdd" if v6 else b"\x08\x00")
    f = eth + ip + seg + bytes(pad)
    return f if snap is None else f[:snap]


def reply(payload=b"", **kw):
    """The same connection's other direction."""
    return frame(payload, src=SERVER, dst=CLIENT, sp=80, dp=40000, **kw)


CH = 128   # the match kernel's piece (kFstPiece)


def payload_lengths(T):
    return [0, 1, max(T - 1, 0), T, T + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 1460]


def filler(n, text, seed):
    """n bytes of lower-case noise with `text` put in at a few places, some of them cut by the end."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = bytearray(rng.integers(97, 123, n, dtype=np.uint8).tobytes())
    for _ in range(1 + n // 40):
        at = int(rng.integers(0, n + 1))
        out[at:at + len(text)] = text[:max(0, n - at)]
    return bytes(out[:n])


def crafted(text, T):
    """The named cases of a pattern that `text` matches, one flow each, over two batches: a list of
    (batch, flow, frame, selected) in packet order, and the number of flows."""
    L = len(text)
    rows, flow = [], 0

    def add(batch, fr_, sel=True, f=None):
        rows.append((batch, flow if f is None else f, fr_, sel))

    for k in range(1, L):                      # a match split at every cut point over two packets
        add(0, frame(b"xx" + text[:k]))
        add(0, frame(text[k:] + b"yy"))
        flow += 1
    a, b = max(1, L // 3), max(2, 2 * L // 3)   # ... over three packets, other flows' packets between them
    add(0, frame(text[:a]))
    add(0, frame(b"junk"), f=flow + 1)
    add(0, frame(text[a:b]))
    add(0, frame(b"junk"), f=flow + 1)
    add(0, frame(text[b:]))
    flow += 2
    for c in text:                             # ... over one packet per byte: the walk back reaches the list's head
        add(0, frame(bytes([c])))
    add(0, frame(b"q"))                        # the match lies wholly in this packet's tail: no second hit
    flow += 1
    add(0, frame(b"zz" + text[:L - 1]))        # ends on the first byte of a packet
    add(0, frame(text[L - 1:] + b"zzzz"))
    flow += 1
    add(0, frame(b"zzz" + text))               # ends on the last byte of a packet
    add(0, frame(b"w"))
    flow += 1
    for cut in (1, L - 1):                     # inside a packet across the piece boundaries
        add(0, frame(b"x" * (CH - cut) + text + b"y" * 9))
        add(0, frame(b"x" * (2 * CH - cut) + text))
        flow += 1
    h = max(1, L // 2)
    add(0, frame(text[:h]))                    # the halves separated by the other direction, a pure ACK,
    add(0, reply(b"HTTP/1.0 200"))             # another flow and an unselected packet
    add(0, frame(b""))
    add(0, frame(b"else"), f=flow + 1)
    add(0, frame(b"!!"), sel=False)
    add(0, frame(text[h:]))
    flow += 2
    add(0, frame(text[:h]))                    # no match across: halves in neighbouring packets of two flows
    add(0, frame(text[h:]), f=flow + 1)
    flow += 2
    add(0, frame(text[:h]))                    # ... and in the two directions of one flow
    add(0, reply(text[h:]))
    flow += 1
    add(0, frame(text[:h]))                    # halves in different batches
    add(1, frame(text[h:]))
    flow += 1
    add(0, reply(b"abc" + text[:L - 1]))       # ... in the reverse direction, one byte behind
    add(1, frame(text))
    add(1, reply(text[L - 1:]))
    flow += 1
    variants = [dict(proto=17), dict(ihl=7), dict(v6=True), dict(vlan=5), dict(tcp_words=8), dict(proto=17, v6=True, vlan=9),
                dict(pad=6), dict(ihl=6, pad=3)]
    for kw in variants:                        # protocols, options, a tag, Ethernet padding
        add(0, frame(b"--" + text[:h], **kw))
        add(1, frame(text[h:] + b"--", **kw))
        flow += 1
    whole = frame(text + text)                 # snapped inside its payload: what it holds, then the next packet
    add(0, whole[:len(whole) - L - (L - h)])
    add(0, frame(text[h:]))
    flow += 1
    add(0, frame(text, proto=1))               # not TCP / UDP: nothing
    add(0, frame(text)[:40])                   # no whole TCP header
    flow += 1
    for ln in payload_lengths(T):              # the lengths, each twice in one stream
        add(0, frame(filler(ln, text, ln)))
        add(1, frame(filler(ln, text, ln + 7)))
    flow += 1
    for sentinel in (0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF, 0xFFFFFFFB):
        add(0, frame(text), f=sentinel)
    add(0, frame(text), f=flow)                # a bad id: flow == the table's size
    add(1, frame(text), f=0x7FFFFFFF)
    return rows, flow


def batches_of(rows):
    """[(frames, ids, select bit list)] per batch of crafted()'s rows."""
    out = []
    for b in sorted({r[0] for r in rows}):
        mine = [r for r in rows if r[0] == b]
        out.append(([r[2] for r in mine], [r[1] for r in mine], [r[3] for r in mine]))
    return out

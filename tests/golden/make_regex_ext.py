"""Builds tests/golden/regex_ext.npz + regex_ext.json: the compiled reference's PAYLOAD
decisions (oracle/_ref, std::regex per packet) for the patterns BT_DFA_EXTENDED adds to the
GPU subset — \\b \\B, POSIX bracket classes, DFAs of more than 254 live states — on crafted
Eth / IPv4 frames whose IP payload is the test string.

    python tests/golden/make_regex_ext.py

Frames: IHL 5 / 6 / 15 x window lengths around every boundary the kernel's walk has (0..9,
31..33, 98..103 and 160: the reference's window is at most 100 bytes) x frame start offsets
of every residue mod 16, strings of word bytes, space, punctuation, \\n, _ and 0x80-0xFF; word
runs that end exactly at window byte 99 with a word byte behind it (`foo\\b` must see the
window's end, not that byte) and word runs that start at byte 0 behind a word byte in the IP
header; and the 256 one-byte windows. Recorded per pattern: the reference's code and
deciding filter per frame, the same with the frames zero-padded to fixed strides of 64 and
128 bytes (255 where a frame does not fit), and one chain with built-in filters around two
extended slots. Only recorded data is written; every pattern must pass and reject a frame."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib as ol  # noqa: E402
from beatrice_amd import synth  # noqa: E402

PROTOCOL, PORT_RANGE, PAYLOAD = 1, 3, 4
CLASSES = ["alpha", "digit", "alnum", "upper", "lower", "space", "blank", "punct", "print", "graph", "cntrl",
           "xdigit", "d", "w", "s"]
WIDE = ["(a|b)*a(a|b){8}", "(ab)*c.{7}d", "\\b(a|b)*a(a|b){7}\\b"]   # > 254 live DFA states
PATTERNS = (["\\bfoo", "foo\\b", "\\Boo", "\\B", "\\b", "(\\b|x)y", "\\bGET\\b|\\bPOST\\b", "^\\b\\w+\\b$",
             "\\b\\d{3}\\b", "[^\\w]\\B.", "a\\b|b\\B", "\\b(GET|POST)\\b"]
            + [f"[[:{c}:]]" for c in CLASSES]
            + ["[[:upper:][:digit:]]+\\b", "[^[:alnum:]_]", "[[:alpha:]_-]{4}", "[^[:space:][:punct:]]{3}$",
               "^[[:xdigit:]]+$", "[[:digit:]]{3}", "(ab)*c.{6}d"]
            + WIDE)
CHAIN = [{"type": PROTOCOL, "expr": "udp", "priority": 3},
         {"type": PAYLOAD, "expr": "\\b(GET|POST)\\b", "priority": 2},
         {"type": PAYLOAD, "expr": "(a|b)*a(a|b){8}", "priority": 1},
         {"type": PORT_RANGE, "expr": "0-40000", "priority": 0}]
IHLS = [5, 6, 15]
WINDOWS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 98, 99, 100, 101, 103, 160]
STRIDES = [64, 128]

WORD = b"abfoGETPOSTxyz0123456789_"
SEP = b" \n-./:,"
HIGH = bytes(range(0x80, 0x100))


def strings(rng, n, count):
    """`count` test strings of n bytes."""
    out = []
    mixes = [WORD + SEP + HIGH, WORD + b" ", b"ab", b"ab" * 8 + b"c", SEP + HIGH, b"0123456789 ", b"fo "]
    words = [b"foo", b"GET", b"POST", b"123", b"xy", b"-y", b"oo", b"1234", b"a", b"b", b"_", b"c123456d", b"ca234567d",
             b"abab", b"\x80\xff", b"AB12", b"dead-beef", b"GET abbabaabab", b"POST/babaaaaaaab"]
    for k in range(count):
        kind = k % 7
        if kind < 3:      # random bytes of one mix
            m = mixes[int(rng.integers(len(mixes)))]
            s = bytes(m[i] for i in rng.integers(0, len(m), n))
        elif kind < 5:    # words and separators
            s = b""
            while len(s) < n:
                j = int(rng.integers(len(SEP)))
                s += words[int(rng.integers(len(words)))] + (SEP[j:j + 1] if rng.integers(3) else b"")
            s = s[:n]
        elif kind == 5:   # a word run that ends at the window's last byte (99 when n > 100), word bytes behind it
            end = min(n, 100)
            w = words[int(rng.integers(4))]
            body = bytes((SEP + b"ab")[i] for i in rng.integers(0, len(SEP) + 2, n))
            s = (body[:max(0, end - len(w) - 1)] + b" " + w)[-end:] if end else b""
            s = (s + b"d0_Z" * 16)[:n]
        else:             # a word run from byte 0
            w = words[int(rng.integers(4))]
            s = (w + b" " + bytes(rng.integers(0, 256, n, dtype=np.uint8)))[:n]
        assert len(s) == n
        out.append(s)
    return out


def frame(ihl, payload, proto, word_before):
    ip = bytearray(ihl * 4)
    ip[0] = 0x40 | ihl
    total = ihl * 4 + len(payload)
    ip[2:4] = total.to_bytes(2, "big")
    ip[8], ip[9] = 64, proto
    ip[12:16] = bytes([10, 1, 2, 3])
    ip[16:20] = bytes([10, 9, 8, ord("a") if word_before else 7])
    for k in range(20, ihl * 4):   # options: word bytes, so the byte before the window is one
        ip[k] = ord("k") if word_before else 0x01
    eth = bytes(range(1, 13)) + b"\x08\x00"
    return eth + bytes(ip) + payload


def main():
    assert ol.ref_available(), "oracle/_ref/libbt_ref.so missing: build() with the reference present"
    rng = np.random.default_rng(20261019)
    frames = []
    for ihl in IHLS:
        for n in WINDOWS:
            short = 14 + 4 * ihl + n <= 64
            for s in strings(rng, n, 42 if short else 16):
                k = len(frames)
                frames.append(frame(ihl, s, 17 if k % 3 else 6, k % 2 == 0))
    for b in range(256):
        frames.append(frame(5, bytes([b]), 17, b % 2 == 0))
    # frame i starts i % 16 bytes past a 16-B boundary
    offs, pos = [], 0
    for i, f in enumerate(frames):
        pos = (pos + 15) // 16 * 16 + i % 16
        offs.append(pos)
        pos += len(f)
    data = np.zeros((pos + 255) // 256 * 256 + 256, np.uint8)
    for o, f in zip(offs, frames):
        data[o:o + len(f)] = np.frombuffer(f, np.uint8)
    desc = synth.make_desc(offs, [len(f) for f in frames])
    n = len(frames)
    assert len(set(o % 16 for o in offs)) == 16

    out = {"data": data, "desc": desc}
    code = np.zeros((len(PATTERNS), n), np.uint8)
    src = np.zeros((len(PATTERNS), n), np.uint8)
    fixed = {}
    for st in STRIDES:
        keep = np.array([i for i, f in enumerate(frames) if len(f) <= st])
        buf = np.zeros(len(keep) * st + 256, np.uint8)
        for j, i in enumerate(keep):
            buf[j * st:j * st + len(frames[i])] = np.frombuffer(frames[i], np.uint8)
        fixed[st] = (keep, buf, np.full((len(PATTERNS), n), 255, np.uint8))
    for p, expr in enumerate(PATTERNS):
        f = [{"type": PAYLOAD, "expr": expr, "priority": 1}]
        code[p], src[p] = ol.ref_filter(data, desc, n, f)
        npass = int((code[p] == 0).sum())
        assert 0 < npass < n, f"/{expr}/ passes {npass} of {n} frames"
        assert set(np.unique(code[p])) <= {0, 1}
        for st, (keep, buf, rec) in fixed.items():
            c, _ = ol.ref_filter(buf, None, len(keep), f, stride=st)
            rec[p, keep] = c
        print(f"{expr:32s} passes {npass:5d} / {n}")
    out["code"], out["src"] = code, src
    for st, (keep, buf, rec) in fixed.items():
        out[f"code{st}"] = rec
    out["chain_code"], out["chain_src"] = ol.ref_filter(data, desc, n, CHAIN)
    np.savez_compressed(os.path.join(HERE, "regex_ext.npz"), **out)
    with open(os.path.join(HERE, "regex_ext.json"), "w") as fh:
        json.dump({"patterns": PATTERNS, "wide": WIDE, "classes": CLASSES, "chain": CHAIN, "strides": STRIDES,
                   "frames": n, "ihl": IHLS, "windows": WINDOWS}, fh, indent=1)
    cc, cs = out["chain_code"], out["chain_src"]
    assert (cc == 0).sum() >= 10 and all(((cc == 1) & (cs == k)).sum() >= 10 for k in range(3))
    print(f"{n} frames, {len(PATTERNS)} patterns, chain codes {np.bincount(cc)}, rejecting filter {np.bincount(cs[cc == 1])}")


if __name__ == "__main__":
    main()

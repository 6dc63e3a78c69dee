"""Classic pcap files built in Python for the pcap tests: global header + records, in any of the
four magics, independent of the code under test."""
import struct

import numpy as np

MAGIC_USEC, MAGIC_NSEC = 0xA1B2C3D4, 0xA1B23C4D
MASK48 = np.uint64((1 << 48) - 1)


def global_header(nanosecond=False, swapped=False, snaplen=65535, linktype=1) -> bytes:
    """24 bytes: magic, version 2.4, thiszone, sigfigs, snaplen, network. `swapped` writes the
    fields in the byte order that is not this machine's (little-endian here: big-endian)."""
    e = ">" if swapped else "<"
    return struct.pack(e + "IHHiIII", MAGIC_NSEC if nanosecond else MAGIC_USEC, 2, 4, 0, 0, snaplen, linktype)


def record(frame: bytes, k: int, swapped=False, orig_extra=0) -> bytes:
    """One record: a timestamp that is distinct per k, incl_len = len(frame), orig_len = incl_len
    + orig_extra (a snapped packet), then the frame."""
    e = ">" if swapped else "<"
    return struct.pack(e + "IIII", 1_700_000_000 + k // 7, (k * 7919 + 13) % 1_000_000, len(frame),
                       len(frame) + orig_extra) + frame


def frames_of(g) -> list:
    """The frames of a golden capture (data + descriptors) as bytes; a descriptor running past
    the data (none of the goldens has one) would be cut."""
    data = g["data"]
    off = (g["desc"] & MASK48).astype(np.int64)
    ln = (g["desc"] >> np.uint64(48)).astype(np.int64)
    return [data[o:o + n].tobytes() for o, n in zip(off, ln)]


def build(frames, nanosecond=False, swapped=False, keep=None) -> bytes:
    """A pcap of `frames` (all of them, or those whose index is in `keep`); every third record
    has orig_len > incl_len. Record k's header depends on k alone, so the pcap of a subset is
    what a verbatim copy of the kept records gives."""
    parts = [global_header(nanosecond, swapped)]
    for k, f in enumerate(frames):
        if keep is None or keep[k]:
            parts.append(record(f, k, swapped, orig_extra=(k % 3 == 0) * (k % 11)))
    return b"".join(parts)

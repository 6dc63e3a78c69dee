"""Crafted frames for the statistics side table's tests (test_flowstat.py, test_gpu_flowstat.py):
builders, and the list that exercises the payload arithmetic, the seen bits and the stamps."""
import numpy as np

import flowtcp_ref as tr


def ip4(proto, l4, src, dst, ttl=64, ihl=5, flags=0, total=None, vlan=0):
    total = 4 * ihl + len(l4) if total is None else total
    ip = bytes([0x40 | ihl, 0]) + total.to_bytes(2, "big") + bytes([0, 0]) + flags.to_bytes(2, "big") + bytes([ttl, proto, 0, 0])
    ip += bytes(src) + bytes(dst) + bytes(4 * max(0, ihl - 5))
    ip = ip[:4 * ihl] if ihl < 5 else ip
    tag = b"".join((b"\x88\xa8" if k == 0 and vlan == 2 else b"\x81\x00") + b"\x00\x05" for k in range(vlan))
    return bytes(12) + tag + b"\x08\x00" + ip + l4


def tcp_hdr(sp, dp, fl, doff=5):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([doff << 4, fl]) + bytes(6)


A, B = [10, 0, 0, 1], [10, 0, 0, 2]


def arithmetic_frames():
    """(frames, what each is for): the payload arithmetic, the seen bits and the stamps."""
    tcp20 = tcp_hdr(1000, 80, tr.ACK | tr.PSH)
    v6 = bytes(12) + b"\x86\xdd" + bytes([0x60, 0, 0, 0, 0, 52, 6, 33]) + bytes(15) + b"\x01" + bytes(15) + b"\x02"
    return [
        (ip4(6, tcp20 + bytes(100), A, B), "IPv4/TCP, 100 bytes of payload"),
        (v6 + tcp_hdr(5, 6, tr.SYN, doff=8) + bytes(32), "IPv6/TCP, payload_length 52, data offset 8: payload 20, a SYN stamp"),
        (ip4(17, bytes([0, 53, 0, 53, 0, 20, 0, 0]) + bytes(12), B, A, ttl=1, vlan=2), "QinQ/IPv4/UDP from the larger endpoint"),
        (ip4(1, bytes(8), A, B, ttl=255), "ICMP"),
        (bytes(12) + b"\x86\xdd" + bytes([0x60, 0, 0, 0, 0, 8, 58, 255]) + bytes(32) + bytes(8), "ICMPv6"),
        (ip4(47, bytes(24), A, B), "GRE: another protocol"),
        (ip4(6, tcp20 + bytes(8), A, B, flags=0x2000), "an IPv4 fragment (MF): addresses only, no payload"),
        (ip4(6, tcp20 + bytes(8), A, B, flags=0x4000), "DF alone is no fragment"),
        (ip4(6, tcp20 + bytes(8), A, B, ihl=6), "IHL 6: options"),
        (ip4(6, tcp20 + bytes(8), A, B, ihl=4), "IHL 4: the L4 header starts inside the addresses' end; no options bit"),
        (ip4(6, tcp20 + bytes(8), A, B, total=30), "total_length below the header sum: 0"),
        (ip4(6, tcp_hdr(1, 2, tr.SYN | tr.ACK, doff=3) + bytes(8), B, A, total=31), "data offset 3, total 31: -1 saturates at 0"),
        (ip4(6, tcp_hdr(1, 2, tr.ACK, doff=15) + bytes(8), A, B), "data offset 15 with a short segment: 0"),
        (ip4(6, tcp_hdr(1, 2, tr.ACK, doff=15) + bytes(8), A, B, total=20 + 61), "data offset 15, one byte of payload"),
        (ip4(6, tcp_hdr(1, 2, tr.ACK | tr.RST), A, B), "RST with ACK: no stamp"),
        (ip4(6, tcp_hdr(1, 2, tr.FIN)[:19], A, B), "a TCP header one byte short: no L4"),
        (ip4(17, bytes(8), A, B, total=0xFFFF), "UDP, total_length 65535 in a snapped capture"),
        (bytes(12) + b"\x08\x06" + bytes(28), "ARP: no IP"),
        (bytes(12) + b"\x81\x00\x00\x01\x81\x00\x00\x02\x81\x00\x00\x03\x08\x00" + bytes(40), "three tags: no IP"),
    ]


def pack_frames(frames):
    """(data, desc): the frames back to back, each at an odd offset."""
    data, desc = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)
        desc.append(len(data) | len(f) << 48)
        data += f
    return np.frombuffer(bytes(data), np.uint8), np.array(desc, np.uint64)

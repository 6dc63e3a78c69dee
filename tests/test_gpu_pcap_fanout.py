"""GPU: tools/pcap_fanout.py in a fresh child process over a pcap written here: about 20
connections with both directions interleaved (some 802.1Q-tagged, some IPv6), non-IP frames and
one fragmented datagram, in chunks of 50 packets. Every output file is compared byte for byte
with the Python oracle's: flow_ref.walk + the bit-serial Toeplitz give each record's queue, and
the records that pass are those bt_pcap_filter (tools/pcap_filter.py's rule) keeps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import pcap_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4
CHUNK = 50


def _eth(et, tags):
    return bytes(6) + bytes([2, 0, 0, 0, 0, 1]) + b"".join(b"\x81\x00" + (100 + t).to_bytes(2, "big") for t in range(tags)) \
        + et.to_bytes(2, "big")


def _v4(src, dst, proto, l4, tags=0, frag=0, ident=0):
    ip = bytes([0x45, 0]) + (20 + len(l4)).to_bytes(2, "big") + ident.to_bytes(2, "big") + frag.to_bytes(2, "big") \
        + bytes([64, proto, 0, 0]) + bytes(src) + bytes(dst)
    return _eth(0x0800, tags) + ip + l4


def _v6(src, dst, nh, l4, tags=0):
    return _eth(0x86DD, tags) + bytes([0x60, 0, 0, 0]) + len(l4).to_bytes(2, "big") + bytes([nh, 64]) + src + dst + l4


def _tcp(sp, dp, payload):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, 0x18, 1, 0, 0, 0, 0, 0]) + payload


def _udp(sp, dp, payload):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + (8 + len(payload)).to_bytes(2, "big") + bytes(2) + payload


def capture():
    """(frames, conn): conn[i] = the connection (or datagram) frame i belongs to, -1 for none."""
    rng = np.random.default_rng(2024)
    frames, conn = [], []
    for step in range(9):
        for c in range(20):
            a = [10, 0, c, 1 + c]
            b = [172, 16, 3 * c % 250, 9]
            a6 = bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(11) + bytes([c + 1])
            b6 = bytes([0x20, 0x01, 0x0d, 0xb8, 0xff]) + bytes(10) + bytes([c + 7])
            sp, dp = 30000 + 17 * c, (80, 443, 53, 8080)[c % 4]
            tags = (0, 0, 1, 2)[c % 4] if c % 5 == 0 else 0
            body = bytes(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8))
            fwd = (step + c) % 2 == 0
            l4 = (_udp if c % 4 == 2 else _tcp)(sp if fwd else dp, dp if fwd else sp, body)
            proto = 17 if c % 4 == 2 else 6
            if c % 3 == 1:
                frames.append(_v6(a6 if fwd else b6, b6 if fwd else a6, proto, l4, tags))
            else:
                frames.append(_v4(a if fwd else b, b if fwd else a, proto, l4, tags))
            conn.append(c)
        frames.append(_eth(0x0806, 0) + bytes(28))   # ARP
        conn.append(-1)
        frames.append(_v6(bytes([0xfe, 0x80]) + bytes(13) + b"\x01", bytes([0xff, 0x02]) + bytes(13) + b"\x01", 58, bytes(8)))
        conn.append(-1)   # ICMPv6: addresses only
        if step < 3:   # one UDP datagram in three fragments: MF, MF + offset, offset
            whole = _udp(5000, 6000, bytes(range(40)))
            piece = whole[16 * step:16 * step + 16] if step < 2 else whole[32:]
            frames.append(_v4([10, 9, 9, 1], [10, 9, 9, 2], 17, piece, frag=(0x2000 if step < 2 else 0) | 2 * step, ident=77))
            conn.append(100)
    frames.append(bytes(10))   # shorter than an Ethernet header
    conn.append(-1)
    return frames, np.array(conn)


def _records(pcap: bytes):
    """The records (header + data) of a pcap written in this machine's byte order."""
    out, at = [], 24
    while at < len(pcap):
        n = int.from_bytes(pcap[at + 8:at + 12], "little")
        out.append(pcap[at:at + 16 + n])
        at += 16 + n
    assert at == len(pcap)
    return out


def _run_tool(tmp_path, fin, extra):
    prefix = str(tmp_path / "q")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_fanout.py"), "--in", str(fin), "--queues", str(K),
                        "--out-prefix", prefix, "--chunk-packets", str(CHUNK), *extra], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    files = [open(f"{prefix}.{q}.pcap", "rb").read() for q in range(K)]
    return json.loads(r.stdout.strip().splitlines()[-1]), files


def _oracle(frames, keep, key, l3_only=False):
    """Per queue: the pcap of the kept records whose frame hashes there, and the class counts."""
    queue, klass = [], []
    for f in frames:
        kb, k = fr.walk(f, l3_only)
        queue.append(int(fr.default_reta(K)[fr.toeplitz(key, kb) & 127]))
        klass.append(k)
    queue, klass = np.array(queue), np.array(klass)
    files = [pcap_util.build(frames, keep=keep & (queue == q)) for q in range(K)]
    return files, queue, [int((klass[keep] == k).sum()) for k in range(5)]


def test_symmetric_fanout_of_a_capture(tmp_path, gpu_ctx):
    frames, conn = capture()
    n = len(frames)
    assert n > 150 and n // CHUNK >= 3
    fin = tmp_path / "in.pcap"
    fin.write_bytes(pcap_util.build(frames))
    gpu_ctx.compile([])
    line, files = _run_tool(tmp_path, fin, ["--symmetric"])
    want, queue, klass = _oracle(frames, np.ones(n, bool), fr.SYMMETRIC_KEY)
    for q in range(K):
        assert files[q] == want[q], f"queue {q}"
    # a connection's two directions, and every fragment of the datagram, share a file
    for c in set(conn.tolist()) - {-1}:
        assert len(set(queue[conn == c].tolist())) == 1, c
    assert len(set(queue[(conn >= 0) & (conn < 100)].tolist())) > 1
    # the files' records, interleaved by capture position, are the capture (no filter: everything passes)
    whole = _records(pcap_util.build(frames))
    pos = {r: i for i, r in enumerate(whole)}
    assert len(pos) == n
    merged = sorted((pos[r], r) for f in files for r in _records(f))
    assert [r for _, r in merged] == _records(gpu_ctx.pcap_filter(np.frombuffer(pcap_util.build(frames), np.uint8))[0]) == whole
    for f in files:
        at = [pos[r] for r in _records(f)]
        assert at == sorted(at) and f[:24] == pcap_util.build(frames)[:24]
    lens = np.array([len(f) for f in frames])
    assert line["packets"] == n == line["passed"] and line["chunks"] == (n + CHUNK - 1) // CHUNK and not line["truncated"]
    assert line["queues"] == [{"packets": int((queue == q).sum()), "bytes": int(lens[queue == q].sum())} for q in range(K)]
    assert list(line["classes"].values()) == klass and klass[fr.NONE] >= 10 and min(klass) > 0


def test_only_passing_records_are_fanned_out(tmp_path, gpu_ctx):
    frames, _ = capture()
    src = pcap_util.build(frames)
    fin = tmp_path / "in.pcap"
    fin.write_bytes(src)
    from beatrice_amd import abi
    gpu_ctx.compile([{"type": abi.PROTOCOL, "expr": "tcp", "priority": 0}])
    try:
        passed = _records(gpu_ctx.pcap_filter(np.frombuffer(src, np.uint8))[0])
    finally:
        gpu_ctx.compile([])
    pos = {r: i for i, r in enumerate(_records(src))}
    keep = np.zeros(len(frames), bool)
    keep[[pos[r] for r in passed]] = True
    assert 0 < keep.sum() < len(frames)
    line, files = _run_tool(tmp_path, fin, ["--filter", "protocol:tcp"])
    want, queue, klass = _oracle(frames, keep, fr.DEFAULT_KEY)
    for q in range(K):
        assert files[q] == want[q], f"queue {q}"
    assert sorted(pos[r] for f in files for r in _records(f)) == np.nonzero(keep)[0].tolist()
    assert line["passed"] == int(keep.sum()) and list(line["classes"].values()) == klass
    assert [x["packets"] for x in line["queues"]] == [int((keep & (queue == q)).sum()) for q in range(K)]

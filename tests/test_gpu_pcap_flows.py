"""GPU: tools/pcap_flows.py in a fresh child process over a pcap written from the fuzz golden and
over a crafted capture of two-way conversations, in three chunks. Every line is compared with the
restatement (flowtab_ref.py) over the whole file: a flow that spans chunks must come out merged."""
import csv
import io
import ipaddress
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import flowtab_ref as ftr
import pcap_util
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("none", "ipv4", "ipv4_l4", "ipv6", "ipv6_l4")


def _rows(want):
    """The tool's lines for the restatement's flows, in order of first packet."""
    out = []
    for f in want["flows"]:
        k, key = int(f["klass"]), f["key"].tobytes()
        alen = 4 if k in (fr.V4, fr.V4_L4) else 16
        ports = k in (fr.V4_L4, fr.V6_L4)
        out.append({"class": NAMES[k], "src": str(ipaddress.ip_address(key[:alen])),
                    "dst": str(ipaddress.ip_address(key[alen:2 * alen])),
                    "sport": int.from_bytes(key[2 * alen:2 * alen + 2], "big") if ports else None,
                    "dport": int.from_bytes(key[2 * alen + 2:2 * alen + 4], "big") if ports else None,
                    "packets": int(f["packets"][0]), "bytes": int(f["bytes"][0]), "packets_rev": int(f["packets"][1]),
                    "bytes_rev": int(f["bytes"][1]), "first": int(f["first"]), "last": int(f["last"])})
    return out


def _run_tool(fin, chunk, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--chunk-packets",
                        str(chunk), *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout, json.loads(r.stderr.strip().splitlines()[-1])


def _csv_rows(text):
    rows = []
    for r in csv.DictReader(io.StringIO(text)):
        rows.append({k: (v if k in ("class", "src", "dst") else None if v == "" else int(v)) for k, v in r.items()})
    return rows


def _passing(gpu_ctx, pcap, filters, n):
    """Which records pass `filters`, by bt_pcap_filter (tools/pcap_filter.py's rule)."""
    gpu_ctx.compile(filters)
    try:
        out = gpu_ctx.pcap_filter(np.frombuffer(pcap, np.uint8))[0]
    finally:
        gpu_ctx.compile([])
    recs, at = {}, 24
    k = 0
    while at < len(pcap):
        m = int.from_bytes(pcap[at + 8:at + 12], "little")
        recs[pcap[at:at + 16 + m]] = k
        at += 16 + m
        k += 1
    assert len(recs) == n   # record k's header depends on k: all distinct
    keep, at = np.zeros(n, bool), 24
    while at < len(out):
        m = int.from_bytes(out[at + 8:at + 12], "little")
        keep[recs[out[at:at + 16 + m]]] = True
        at += 16 + m
    return keep


def test_fuzz_in_three_chunks(tmp_path, gpu_ctx):
    from beatrice_amd import abi
    g, _ = load_golden("fuzz")
    frames = pcap_util.frames_of(g)
    n = len(frames)
    pcap = pcap_util.build(frames)
    fin = tmp_path / "fuzz.pcap"
    fin.write_bytes(pcap)
    lens = [len(f) for f in frames]
    keep = _passing(gpu_ctx, pcap, [{"type": abi.PROTOCOL, "expr": "udp", "priority": 0}], n)
    assert 0 < keep.sum() < n
    for extra, flags, sel in (([], 0, None), (["--bidirectional"], ftr.BIDIRECTIONAL, None),
                              (["--filter", "protocol:udp", "--bidirectional", "--l3-only"],
                               ftr.BIDIRECTIONAL | ftr.L3_ONLY, fr.pack_bits(keep))):
        inputs, nbytes, klass = fr.key_of_rec(g["rec"], bool(flags & ftr.L3_ONLY))
        want = ftr.expected(inputs, nbytes, klass, lens, flags, sel)
        text, totals = _run_tool(fin, 3000, extra)
        assert _csv_rows(text) == _rows(want), extra
        assert totals == {"packets": n, "selected": want["result"]["n_selected"], "no_key": want["result"]["none_packets"],
                          "chunks": 3, "truncated": 0, "flows": want["result"]["n_flows"]}
    assert want["result"]["n_flows"] > 10


def _eth(et):
    return bytes(6) + bytes([2, 0, 0, 0, 0, 1]) + et.to_bytes(2, "big")


def _v4(src, dst, proto, l4):
    return _eth(0x0800) + bytes([0x45, 0]) + (20 + len(l4)).to_bytes(2, "big") + bytes(4) + bytes([64, proto, 0, 0]) \
        + bytes(src) + bytes(dst) + l4


def _v6(src, dst, nh, l4):
    return _eth(0x86DD) + bytes([0x60, 0, 0, 0]) + len(l4).to_bytes(2, "big") + bytes([nh, 64]) + src + dst + l4


def _tcp(sp, dp, payload):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, 0x18, 1, 0, 0, 0, 0, 0]) + payload


def _udp(sp, dp, payload):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + (8 + len(payload)).to_bytes(2, "big") + bytes(2) + payload


def conversations():
    """Six conversations with both directions interleaved over the whole capture (so each spans
    the chunks), ARP in between."""
    rng = np.random.default_rng(7)
    frames = []
    for step in range(24):
        for c in range(6):
            a, b = [10, 0, c, 1 + c], [172, 16, c, 9]
            a6 = bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(11) + bytes([c + 1])
            b6 = bytes([0x20, 0x01, 0x0d, 0xb8, 0xff]) + bytes(10) + bytes([c + 7])
            sp, dp = 30000 + c, (80, 443, 53)[c % 3]
            body = bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8))
            fwd = (step * 5 + c) % 3 != 0
            l4 = (_udp if c % 3 == 2 else _tcp)(sp if fwd else dp, dp if fwd else sp, body)
            proto = 17 if c % 3 == 2 else 6
            if c % 2:
                frames.append(_v6(a6 if fwd else b6, b6 if fwd else a6, proto, l4))
            else:
                frames.append(_v4(a if fwd else b, b if fwd else a, proto, l4))
        frames.append(_eth(0x0806) + bytes(28))
    return frames


def test_two_way_conversations_in_three_chunks(tmp_path, gpu_ctx):
    from beatrice_amd import abi
    frames = conversations()
    n = len(frames)
    assert n == 168
    pcap = pcap_util.build(frames)
    fin = tmp_path / "conv.pcap"
    fin.write_bytes(pcap)
    keep = _passing(gpu_ctx, pcap, [{"type": abi.PROTOCOL, "expr": "tcp", "priority": 0}], n)
    assert 0 < keep.sum() < n - 24
    for extra, flags, sel, nflows in ((["--bidirectional"], ftr.BIDIRECTIONAL, None, 6), ([], 0, None, 12),
                                      (["--filter", "protocol:tcp", "--bidirectional"], ftr.BIDIRECTIONAL, fr.pack_bits(keep), None),
                                      (["--filter", "protocol:tcp"], 0, fr.pack_bits(keep), None)):
        want = ftr.of_frames(frames, flags, sel)
        if nflows is None:   # which conversations the filter keeps is the filter's business: some, not all
            nflows = want["result"]["n_flows"]
            assert 0 < nflows < (6 if flags else 12) and want["result"]["none_packets"] == 0
        assert want["result"]["n_flows"] == nflows and want["result"]["none_packets"] == (0 if sel is not None else 24)
        text, totals = _run_tool(fin, 60, extra)
        rows = _csv_rows(text)
        assert rows == _rows(want), extra
        assert totals["chunks"] == 3 and totals["flows"] == nflows and totals["selected"] == want["result"]["n_selected"]
        if flags:   # both directions counted, and every conversation spans all three chunks
            assert all(r["packets"] > 0 and r["packets_rev"] > 0 and r["first"] < 60 and r["last"] >= 120 for r in rows)
    # json lines and --top: the two largest conversations, largest first
    text, _ = _run_tool(fin, 60, ["--bidirectional", "--format", "json", "--top", "2"])
    got = [json.loads(x) for x in text.strip().splitlines()]
    every = sorted(_rows(ftr.of_frames(frames, ftr.BIDIRECTIONAL)), key=lambda r: (-(r["bytes"] + r["bytes_rev"]), r["first"]))
    assert got == every[:2]

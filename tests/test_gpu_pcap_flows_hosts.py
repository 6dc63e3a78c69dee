"""GPU: tools/pcap_flows.py --track --hosts prints the endpoint view from the device
(bt_flow_track_hosts_device): on a small crafted capture (a server every client talks to, a client
that only sends SYNs, an IPv6 pair, a frame with both addresses equal) the csv is the restatement's
(flowtrack_ref + flowtcp_ref for the tracker, flowhosts_ref for the hosts, formatted here), with and
without --tcp and --top, and the output without --hosts is what it was."""
import ipaddress
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import flowhosts_ref as fh
import flowtab_ref as ftr
import flowtcp_ref as tr
import flowtrack_ref as fkr
import pcap_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "pcap_flows.py")
SERVER = [10, 0, 0, 2]
STATES = ("none", "opening", "established", "closing", "closed", "reset", "midstream")
CHUNK = 14


def _tcp4(src, dst, sp, dp, flags, pad=0):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + struct.pack(">HH", sp, dp) + bytes(8) + bytes([0x50, flags]) + bytes(6 + pad)


def _udp6(src, dst, sp, dp, pad=0):
    ip = bytes([0x60, 0, 0, 0, 0, 8 + pad, 17, 64]) + src + dst
    return bytes(12) + b"\x86\xdd" + ip + struct.pack(">HHHH", sp, dp, 8 + pad, 0) + bytes(pad)


def frames():
    out = []
    six_a, six_b = fh.v6(0x01020304 << 96), fh.v6((0x20010DB8 << 96) + 7)
    for rnd in range(6):
        for c in range(9):   # client c: c % 4 + 1 rounds; SYN, SYN|ACK back, then ACKs; client 8 only ever sends SYNs
            client = [10, 0, 1, c]
            if rnd > c % 4 and c != 8:
                continue
            if c == 8 or rnd == 0:
                out.append(_tcp4(client, SERVER, 2000 + c, 443, tr.SYN, pad=c))
            if c != 8 and rnd == 0:
                out.append(_tcp4(SERVER, client, 443, 2000 + c, tr.SYN | tr.ACK))
            elif c != 8:
                out.append(_tcp4(client, SERVER, 2000 + c, 443, tr.ACK | (tr.FIN if rnd == c % 4 else 0), pad=3 * rnd))
        out.append(_udp6(six_a, six_b, 53, 5000 + rnd, pad=rnd))
        if rnd % 2:
            out.append(_tcp4([1, 2, 3, 4], [1, 2, 3, 4], 7, 7, tr.RST))   # both addresses equal; 1.2.3.4 beside 0102:0304::
    return out


def _stamps(n):
    k = np.arange(n, dtype=np.uint64)
    return (np.uint64(1_700_000_000) + k // np.uint64(7)) * np.uint64(1_000_000) + (k * np.uint64(7919) + np.uint64(13)) % np.uint64(1_000_000)


def restated(fs, flags, with_tcp):
    """The host records the tool should print, from the Python walk over the frames."""
    keys = fr.key_of_frames(fs, False)
    tcp, fl = tr.tcp_of_frames(fs)
    dirs = tr.directions(*keys, flags)
    lens = np.array([len(f) for f in fs], np.int64)
    ts = _stamps(len(fs))
    ref, side = fkr.Tracker(len(fs), flags), np.zeros(len(fs), tr.TCP_REC)
    for lo in range(0, len(fs), CHUNK):
        hi = min(len(fs), lo + CHUNK)
        wid = ref.update(keys[0][lo:hi], keys[1][lo:hi], keys[2][lo:hi], lens[lo:hi], None, ts[lo:hi])["flow_id"]
        tr.update(side, wid, tcp[lo:hi], fl[lo:hi], dirs[lo:hi])
    recs = ref.records()
    return fh.expected(recs, side if with_tcp else None, flags, 2 * len(fs), fh.auto_slots(len(fs)))


def csv_of(hosts, with_tcp, top=0, by=None):
    cols = ["address", "flows_src", "flows_dst", "packets_sent", "bytes_sent", "packets_received", "bytes_received", "first_seen", "last_seen"]
    if with_tcp:
        cols += ["tcp_" + s for s in STATES] + ["syn_flows_sent", "syn_flows_received", "syn", "fin", "rst"]
    rows = []
    for h in hosts:
        addr = ipaddress.ip_address(bytes(h["addr"])[:4 if h["family"] == 4 else 16])
        stamp = lambda v: f"{int(v) // 1_000_000}.{int(v) % 1_000_000:06d}"   # noqa: E731
        r = [str(addr), int(h["flows"][0]), int(h["flows"][1]), int(h["packets"][0]), int(h["bytes"][0]), int(h["packets"][1]),
             int(h["bytes"][1]), stamp(h["first_ts"]), stamp(h["last_ts"])]
        if with_tcp:
            r += [int(x) for x in h["tcp_state"]] + [int(x) for x in h["syn_flows"]] + [int(h["syn_packets"]), int(h["fin_packets"]), int(h["rst_packets"])]
        rows.append(r)
    if top:
        key = {"bytes": lambda r: r[4] + r[6], "packets": lambda r: r[3] + r[5], "flows": lambda r: r[1] + r[2]}[by or "bytes"]
        rows = sorted(rows, key=lambda r: -key(r))[:top]
    return "\n".join([",".join(cols)] + [",".join(str(x) for x in r) for r in rows]) + "\n"


def _run(fin, extra, ok=True):
    r = subprocess.run([sys.executable, TOOL, "--in", str(fin), "--chunk-packets", str(CHUNK), *extra], capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def test_hosts_from_the_device(tmp_path, gpu_ctx):
    fs = frames()
    fin = tmp_path / "hosts.pcap"
    fin.write_bytes(pcap_util.build(fs))
    assert len(fs) > 3 * CHUNK
    for flags, extra in ((ftr.BIDIRECTIONAL, ["--bidirectional"]), (0, [])):
        want = restated(fs, flags, True)
        hosts = want["hosts"]
        assert want["result"]["n_hosts"] == 13 and want["result"]["hosts_v6"] == 2
        server = hosts[[bytes(h["addr"][:4]) == bytes(SERVER) for h in hosts]][0]
        assert server["flows"].sum() == (9 if flags else 17)   # one flow per client, or one per direction
        assert flags == 0 or server["tcp_state"][1] == 1       # the SYN-only client's flow is "opening"
        got = _run(fin, ["--track", "--hosts", "--tcp", *extra])
        assert got.stdout == csv_of(hosts, True)
        assert '"hosts": 13' in got.stderr and '"hosts_v6": 2' in got.stderr
        assert _run(fin, ["--track", "--hosts", *extra]).stdout == csv_of(restated(fs, flags, False)["hosts"], False)
        for by in ("bytes", "packets", "flows"):
            assert _run(fin, ["--track", "--hosts", "--tcp", "--top", "4", "--by", by, *extra]).stdout == csv_of(hosts, True, 4, by), by
        assert _run(fin, ["--track", "--hosts", "--top", "3", *extra]).stdout == csv_of(restated(fs, flags, False)["hosts"], False, 3)
    js = _run(fin, ["--track", "--hosts", "--format", "json", "--top", "1"]).stdout
    assert js.count("\n") == 1 and '"address": "10.0.0.2"' in js
    # without --hosts nothing has changed: the tracked output is the default path's, byte for byte
    assert _run(fin, ["--track", "--bidirectional"]).stdout == _run(fin, ["--bidirectional"]).stdout
    assert "--hosts: only with --track" in _run(fin, ["--hosts"], ok=False).stderr
    assert "--hosts: only with --track" in _run(fin, ["--track", "--hosts", "--idle", "5"], ok=False).stderr
    assert "--hosts --by" in _run(fin, ["--track", "--hosts", "--top", "3", "--by", "syn", "--tcp"], ok=False).stderr
    assert "--by flows: only with --hosts" in _run(fin, ["--track", "--top", "3", "--by", "flows"], ok=False).stderr

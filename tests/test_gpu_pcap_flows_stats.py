"""GPU: tools/pcap_flows.py --track --stats on a small synthetic capture built here: the statistics
columns against the restatement in flowstat_ref.py applied to each flow's packets, with an expiry
in the middle of the capture (the statistics leave with the flow, through
bt_flow_track_side_move_device) and a flow that comes back as a new one."""
import csv
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import flowstat_ref as sr
import flowtab_ref as ftr
import flowtcp_ref as tr
import pcap_util
from flowstat_cases import ip4, tcp_hdr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = [10, 0, 0, 1], [10, 0, 0, 2]
NAMES = ((sr.SEEN_TCP, "tcp"), (sr.SEEN_UDP, "udp"), (sr.SEEN_ICMP, "icmp"), (sr.SEEN_ICMP6, "icmp6"), (sr.SEEN_OTHER, "other"))


def tcp(conv, d, fl, payload=0, ttl=64, vlan=0):
    src, dst, sp, dp = (A, B, 1000 + conv, 80) if d == 0 else (B, A, 80, 1000 + conv)
    return ip4(6, tcp_hdr(sp, dp, fl) + bytes(payload), src, dst, ttl=ttl, vlan=vlan)


def udp(d, payload, ttl):
    src, dst = (A, B) if d == 0 else (B, A)
    return ip4(17, bytes([0, 53, 0, 53]) + (8 + payload).to_bytes(2, "big") + bytes(2) + bytes(payload), src, dst, ttl=ttl)


def capture():
    """56 (conversation, frame) pairs; pcap_util stamps packet k with second k // 7, so a chunk of 14 is
    two seconds. Conversation 0 (a handshake and data) and 2 (ICMP) end in the first chunk and age out
    behind the second and the third with --idle 2.5; 1 (DNS, both ways) and 3 (a tagged TCP connection from the
    third chunk on, opened by the larger endpoint) live to the end; 0 comes back with the last packet."""
    S, K, P = tr.SYN, tr.ACK, tr.PSH
    p = {0: (0, tcp(0, 0, S, ttl=64)), 1: (0, tcp(0, 1, S | K, ttl=57)), 2: (0, tcp(0, 0, K)), 3: (0, tcp(0, 0, K | P, 300)),
         4: (0, tcp(0, 1, K | P, 1200, ttl=57)), 6: (2, ip4(1, bytes(8) + bytes(40), A, B, ttl=128)), 9: (2, ip4(1, bytes(8) + bytes(56), A, B, ttl=127)),
         28: (3, tcp(3, 1, S, ttl=250, vlan=1)), 29: (3, tcp(3, 0, S | K, ttl=60, vlan=1)), 31: (3, tcp(3, 1, K, ttl=249, vlan=1)),
         55: (0, tcp(0, 0, S, ttl=63))}
    for k in (5, 12, 20, 26, 33, 40, 47, 54):
        p[k] = (1, udp(k % 2, 20 + k, 30 + k))
    for k in range(56):
        if k not in p:   # filler: conversation 1 in the first half (so that it never goes idle), 3 in the second
            p[k] = (1, udp(k % 2, k, 64)) if k < 28 else (3, tcp(3, k % 2, K | P, 10 * (k % 5), ttl=60 + k % 3, vlan=1))
    return [p[k] for k in range(56)]


def stamp(k):
    return (1_700_000_000 + k // 7) * 1_000_000 + (k * 7919 + 13) % 1_000_000


def expected(pk):
    """The --stats columns of the flow made of the packets pk = [(k, frame)], by the restatement."""
    frames = [f for _, f in pk]
    facts = sr.facts_of_frames(frames)
    dirs = tr.directions(*fr.key_of_frames(frames), ftr.BIDIRECTIONAL)
    table = np.zeros(1, sr.STAT_REC)
    sr.update(table, np.zeros(len(pk), np.uint32), facts, dirs, np.array([stamp(k) for k, _ in pk], np.uint64))
    t = table[0]
    seen = int(t["seen"]) | int(t["seen"]) >> 16
    want = {"protocols": "+".join(n for b, n in NAMES if seen & b), "proto_max": str(int(t["proto_max"])),
            "packets": str(int((dirs == 0).sum())), "packets_rev": str(int((dirs == 1).sum())), "first": str(pk[0][0]), "last": str(pk[-1][0])}
    for d, suffix in enumerate(("", "_rev")):
        lens = [len(f) for f, x in zip(frames, dirs) if x == d]
        for c in ("len_min", "len_mean", "len_max", "len_stddev", "ttl_min", "ttl_max"):
            want[c + suffix] = ""
        if lens:
            n, b, sq = len(lens), sum(lens), sum(x * x for x in lens)
            assert sq == int(t["len_sq"][d])
            want["len_min" + suffix], want["len_max" + suffix] = str(sr.U32 - int(t["len_min_c"][d])), str(int(t["len_max"][d]))
            want["len_mean" + suffix], want["len_stddev" + suffix] = f"{b / n:.3f}", f"{math.sqrt(n * sq - b * b) / n:.3f}"
            want["ttl_min" + suffix], want["ttl_max" + suffix] = str(sr.U32 - int(t["ttl_min_c"][d])), str(int(t["ttl_max"][d]))
        want["payload_bytes" + suffix], want["payload_packets" + suffix] = str(int(t["payload_bytes"][d])), str(int(t["payload_packets"][d]))
    r = sr.rtt(t)
    want["initiator"] = ("fwd", "rev")[r["initiator"]] if r["has_initiator"] else ""
    want["rtt_server"] = str(r["rtt_server"]) if r["server_valid"] else ""
    want["rtt_client"] = str(r["rtt_client"]) if r["client_valid"] else ""
    return want


def _run(fin, extra, ok=True):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--chunk-packets", "14", *extra],
                       capture_output=True, text=True, timeout=120)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr
    return list(csv.DictReader(io.StringIO(r.stdout))), json.loads(r.stderr.strip().splitlines()[-1])


def test_stats_columns_with_an_expiry_and_a_reopened_flow(tmp_path, gpu_ctx):
    cap = capture()
    fin = tmp_path / "stats.pcap"
    fin.write_bytes(pcap_util.build([f for _, f in cap]))
    by = {c: [(k, f) for k, (conv, f) in enumerate(cap) if conv == c] for c in range(4)}
    # the restatement by hand, once: conversation 0's first life
    w = expected(by[0][:-1])
    assert (w["protocols"], w["len_min"], w["len_max"], w["len_min_rev"], w["len_max_rev"]) == ("tcp", "54", "354", "54", "1254")
    assert (w["ttl_min"], w["ttl_max"], w["ttl_min_rev"], w["payload_bytes"], w["payload_bytes_rev"]) == ("64", "64", "57", "300", "1200")
    assert (w["initiator"], w["rtt_server"], w["rtt_client"]) == ("fwd", "7919", "7919") and w["len_mean"] == f"{(54 + 54 + 354) / 3:.3f}"
    # one wait, every flow at the end, in order of first packet: 0, 1, 2, 3
    rows, totals = _run(fin, ["--bidirectional", "--track", "--stats"])
    assert totals["flows"] == 4 and totals["chunks"] == 4 and len(rows) == 4
    for row, c in zip(rows, range(4)):
        want = expected(by[c])
        assert {k: row[k] for k in want} == want, (c, row, want)
    assert [r["protocols"] for r in rows] == ["tcp", "udp", "icmp", "tcp"] and rows[3]["initiator"] == "rev" and rows[2]["initiator"] == ""
    assert rows[3]["rtt_server"] == "7919" and rows[3]["rtt_client"] == str(2 * 7919)
    # --idle 2.5: conversations 0 and 2 age out behind the second and the third chunk and are printed first, with the
    # statistics that left with them; 1 and 3 keep theirs through the renumbering; 0's last packet is a new flow
    aged, totals = _run(fin, ["--bidirectional", "--track", "--stats", "--idle", "2.5"])
    assert totals["flows"] == 5
    for row, pk in zip(aged, (by[0][:-1], by[2], by[1], by[3], by[0][-1:])):
        want = expected(pk)
        assert {k: row[k] for k in want} == want, (row, want)
    assert (aged[4]["initiator"], aged[4]["rtt_server"], aged[4]["payload_packets"], aged[4]["ttl_max"]) == ("fwd", "", "0", "63")
    # with --tcp the TCP columns stand in front of the statistics, and both follow their flows
    both, _ = _run(fin, ["--bidirectional", "--track", "--tcp", "--stats", "--idle", "2.5"])
    assert [{k: v for k, v in r.items() if not k.startswith("tcp_") and k not in ("syn", "fin", "rst")} for r in both] == [dict(r) for r in aged]
    assert [r["tcp_state"] for r in both] == ["established", "none", "none", "established", "opening"]
    # unidirectional: nothing in the reverse columns, no RTT columns; the answers are flows of their own
    uni, totals = _run(fin, ["--track", "--stats"])
    assert totals["flows"] == 7 and "initiator" not in uni[0] and all(r["len_min_rev"] == "" and r["payload_bytes_rev"] == "0" for r in uni)
    # without --stats the tool prints what it always printed
    plain, _ = _run(fin, ["--bidirectional", "--track", "--idle", "2.5"])
    assert [dict(r) for r in plain] == [{k: v for k, v in r.items() if k in plain[0]} for r in aged]
    assert "protocols" not in plain[0] and list(plain[0]) == list(aged[0])[:len(plain[0])]
    r = _run(fin, ["--stats"], ok=False)
    assert r.returncode != 0 and "--stats: only with --track" in r.stderr
    r = _run(fin, ["--track", "--stats", "--top", "3"], ok=False)
    assert r.returncode != 0 and "--stats" in r.stderr

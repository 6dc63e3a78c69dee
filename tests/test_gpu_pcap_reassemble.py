"""GPU: tools/pcap_sessions.py --stream HELLO --reassemble as a child process over a capture written here,
with swapped, duplicated and hole-filling segments: the arrival-order run selects fewer sessions, and one
that is wrong; the reassembling run selects exactly the connections whose true byte stream holds HELLO.
tools/pcap_flows.py --track --reasm HELLO prints the planted per-direction counts, also when a connection ages
out between two chunks and the others' records move in the middle of their streams."""
import csv
import io
import json
import os
import struct
import subprocess
import sys

import pytest

import flowtcpseq_cases as tc
import pcap_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "pcap_sessions.py")


def capture():
    """(frames, the connection of each, the connections whose true stream holds HELLO, those the arrival order shows it in)."""
    def seg(k, off, data, **kw):
        return k, tc.tcp(1000 * (k + 1) + off, payload=data, sp=40001 + k, **kw)

    rows = [seg(0, 6, b"LOdef"), seg(1, 0, b"xHE"), seg(2, 0, b"HE"), seg(3, 0, b"..HE"), seg(4, 0, b"HEL", proto=17),
            seg(0, 0, b"abcHEL"),                                   # 0: swapped
            seg(1, 4, b"LOy"), seg(1, 3, b"L"),                     # 1: the hole's filler comes last
            seg(2, 2, b"LL"), seg(2, 2, b"LL"), seg(2, 4, b"O"),    # 2: a duplicate in the middle
            seg(3, 4, b"LLO.."),                                    # 3: in order
            seg(4, 0, b"LO", proto=17),                             # 4: UDP, in arrival order by the stream matcher
            seg(5, 0, b"xxHEL"), seg(5, 6, b"LOyy"),                # 5: a byte is missing inside what reads HELLO
            seg(6, 0, b"HELL"), seg(6, 4, b"..O")]                  # 6: nothing
    return [f for _, f in rows], [k for k, _ in rows], {0, 1, 2, 3, 4}, {3, 4, 5}


def run_tool(tmp_path, extra):
    frames, _, _, _ = capture()
    fin, fout = tmp_path / "in.pcap", tmp_path / "out.pcap"
    fin.write_bytes(pu.build(frames))
    r = subprocess.run([sys.executable, TOOL, "--in", str(fin), "--out", str(fout), "--bidirectional", "--stream", "HELLO", *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), fout.read_bytes()


def test_reassembly_selects_exactly_the_generators_sessions(tmp_path):
    frames, conn, true_set, arrival_set = capture()
    plain, out = run_tool(tmp_path, [])
    assert out == pu.build(frames, keep=[k in arrival_set for k in conn]) and plain["marked_flows"] == len(arrival_set)
    res, out = run_tool(tmp_path, ["--reassemble"])
    assert out == pu.build(frames, keep=[k in true_set for k in conn])
    assert plain["marked_flows"] < res["marked_flows"] == len(true_set)
    assert res["reasm_hit_packets"] == 4 and res["stream_hit_packets"] == 1 and res["holes"] == 1 and res["dup_packets"] == 1
    assert res["late_packets"] == 0 and res["far_packets"] == 0 and res["reasm_packets"] == 14 and res["stream_packets"] == 2


def test_with_a_filter_hit_packets_stays_the_verdicts(tmp_path):
    """A filter that passes nothing beside --stream --reassemble: the sessions are the reassembly's and the stream's,
    hit_packets counts the verdict's hits alone, whichever matcher marked a flow."""
    frames, conn, true_set, _ = capture()
    res, out = run_tool(tmp_path, ["--reassemble", "--filter", "payload:QQQQ"])
    assert out == pu.build(frames, keep=[k in true_set for k in conn])
    assert res["hit_packets"] == 0 and res["reasm_hit_packets"] == 4 and res["stream_hit_packets"] == 1 and res["marked_flows"] == len(true_set)
    plain, _ = run_tool(tmp_path, ["--filter", "payload:QQQQ"])
    assert plain["hit_packets"] == 0 and plain["stream_hit_packets"] == 3 and plain["marked_flows"] == 3


def test_reassemble_with_skip_retransmits_is_an_argument_error(tmp_path):
    r = subprocess.run([sys.executable, TOOL, "--in", str(tmp_path / "none"), "--out", str(tmp_path / "out"), "--stream", "HELLO",
                        "--reassemble", "--skip-retransmits"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "supersedes --skip-retransmits" in r.stderr
    r = subprocess.run([sys.executable, TOOL, "--in", str(tmp_path / "none"), "--out", str(tmp_path / "out"), "--filter", "PROTOCOL:TCP",
                        "--reassemble"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "goes with --stream" in r.stderr


FLOWS = os.path.join(ROOT, "tools", "pcap_flows.py")
NAMES = ("reasm_packets", "reasm_hits", "holes", "hole_bytes", "dup_packets", "dup_bytes", "late_packets", "late_bytes", "delivered_to")


def flows_of(path, extra):
    r = subprocess.run([sys.executable, FLOWS, "--in", str(path), "--bidirectional", "--track", "--reasm", "HELLO", *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = list(csv.DictReader(io.StringIO(r.stdout)))
    assert all(x[n + "_rev"] in ("0", "") for x in rows for n in NAMES), "nothing was sent the other way"
    return [int(x["sport"]) for x in rows], {int(x["sport"]): [x[n] for n in NAMES] for x in rows}, r.stdout


def test_pcap_flows_prints_the_planted_counts(tmp_path):
    frames, _, _, _ = capture()
    fin = tmp_path / "in.pcap"
    fin.write_bytes(pu.build(frames))
    _, got, text = flows_of(fin, [])
    want = {40001: [2, 1, 0, 0, 0, 0, 0, 0, 5], 40002: [3, 1, 0, 0, 0, 0, 0, 0, 7], 40003: [3, 1, 0, 0, 1, 2, 0, 0, 5],
            40004: [2, 1, 0, 0, 0, 0, 0, 0, 9], 40005: [0, 0, 0, 0, 0, 0, 0, 0, ""], 40006: [2, 0, 1, 1, 0, 0, 0, 0, 10],
            40007: [2, 0, 0, 0, 0, 0, 0, 0, 7]}
    assert got == {k: [str(x) for x in v] for k, v in want.items()}
    plain = subprocess.run([sys.executable, FLOWS, "--in", str(fin), "--bidirectional", "--track"], capture_output=True, text=True, timeout=120)
    width = len(plain.stdout.splitlines()[0].split(","))   # without the option the output is as before: the new columns come last
    assert "reasm_packets" not in plain.stdout
    assert [ln.split(",") for ln in plain.stdout.splitlines()] == [ln.split(",")[:width] for ln in text.splitlines()]
    both = subprocess.run([sys.executable, FLOWS, "--in", str(fin), "--bidirectional", "--track", "--seq", "--reasm", "HELLO"],
                          capture_output=True, text=True, timeout=120)
    assert both.returncode == 0 and "old_packets" in both.stdout.splitlines()[0] and both.stdout.splitlines()[0].endswith("delivered_to_rev")


def test_the_reassembly_records_follow_a_real_expire(tmp_path):
    """--idle: connection A falls idle and ages out behind the second chunk; its record leaves with it and those of B
    and C move down by the expire's remap (bt_flow_track_side_move_device with rec_bytes = 128) in the middle of
    their streams, B with a matcher state and a position: the counts are those of the run without --idle."""
    def seg(k, off, data):
        return tc.tcp(1000 * (k + 1) + off, payload=data, sp=40001 + k)

    timed = [(0.0, seg(0, 0, b"xHEL")), (0.1, seg(0, 4, b"LO")), (0.2, seg(1, 0, b"abc")), (0.3, seg(0, 6, b"zz")),
             (10.0, seg(1, 6, b"LO")), (10.1, seg(1, 3, b"HEL")), (10.2, seg(2, 0, b"HE")), (10.3, seg(2, 2, b"LLO")),
             (11.0, seg(2, 5, b"x")), (11.1, seg(1, 8, b"HELLO")), (11.2, seg(2, 6, b"HELLO")), (11.3, seg(1, 13, b"q"))]
    fin = tmp_path / "idle.pcap"
    fin.write_bytes(pu.global_header() + b"".join(
        struct.pack("<IIII", 1_700_000_000 + int(t), round(t % 1 * 1_000_000), len(f), len(f)) + f for t, f in timed))
    order, idle, _ = flows_of(fin, ["--chunk-packets", "4", "--idle", "5"])
    _, plain, _ = flows_of(fin, ["--chunk-packets", "4"])
    assert order == [40001, 40002, 40003], "the idle connection is printed when it ages out"
    want = {40001: [3, 1, 0, 0, 0, 0, 0, 0, 8], 40002: [5, 2, 0, 0, 0, 0, 0, 0, 14], 40003: [4, 2, 0, 0, 0, 0, 0, 0, 11]}
    assert idle == plain == {k: [str(x) for x in v] for k, v in want.items()}

"""GPU: the TCP sequence classification in the two tools, as child processes over a capture written here.
tools/pcap_sessions.py --stream HELLO over HE, LL, LL again (the same sequence number), O in one
connection: the arrival-order stream reads HELLLLO, so only --skip-retransmits selects it; a second
connection that sends ab twice is selected for abab only without the option. tools/pcap_flows.py --track
--seq prints the planted counts."""
import csv
import io
import json
import os
import subprocess
import sys

import pytest

import flowtcpseq_cases as tc
import pcap_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def capture():
    """(frames, the connection of each): 0 HELLO with a retransmit, 1 ab twice, 2 a loss, an overlap and a reply."""
    a, b, c = dict(sp=40001), dict(sp=40002), dict(sp=40003)
    rows = [(0, tc.tcp(99, 0, tc.SYN, **a)), (1, tc.tcp(4999, 0, tc.SYN, **b)), (0, tc.tcp(100, payload=b"HE", **a)),
            (1, tc.tcp(5000, payload=b"ab", **b)), (0, tc.tcp(102, payload=b"LL", **a)), (2, tc.tcp(tc.M32 - 9, 20, **c)),
            (0, tc.tcp(0, 0, tc.ACK, rev=True, **a)), (0, tc.tcp(102, payload=b"LL", **a)), (1, tc.tcp(5000, payload=b"ab", **b)),
            (2, tc.tcp(tc.M32 - 9 + 30, 20, **c)), (0, tc.tcp(104, payload=b"O", **a)), (2, tc.tcp(tc.M32 - 9 + 40, 20, **c)),
            (2, tc.tcp(700, 5, rev=True, **c)), (2, tc.tcp(705, 5, rev=True, **c)), (2, tc.tcp(700, 5, rev=True, **c))]
    return [f for _, f in rows], [k for k, _ in rows]


def run_tool(tmp_path, tool, extra):
    frames, _ = capture()
    fin, fout = tmp_path / "in.pcap", tmp_path / "out.pcap"
    fin.write_bytes(pu.build(frames))
    out = ["--out", str(fout)] if tool == "pcap_sessions.py" else []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--in", str(fin), *out, "--bidirectional", *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout, fout.read_bytes() if out else None


def test_the_sequence_spaces_follow_a_real_expire(tmp_path):
    """--idle: the connection that sent ab twice falls idle and ages out behind the second chunk
    (bt_flow_track_expire_device), its record leaves with it and the others move down by the expire's remap
    (bt_flow_track_side_move_device with rec_bytes = 128) in the middle of their streams: the counts are
    those of the run without --idle."""
    import struct
    a, b, c = dict(sp=40001), dict(sp=40002), dict(sp=40003)
    timed = [(0.0, tc.tcp(4999, 0, tc.SYN, **b)), (0.1, tc.tcp(5000, payload=b"ab", **b)), (0.2, tc.tcp(99, 0, tc.SYN, **a)),
             (0.3, tc.tcp(5000, payload=b"ab", **b)),
             (10.0, tc.tcp(100, payload=b"HE", **a)), (10.1, tc.tcp(102, payload=b"LL", **a)), (10.2, tc.tcp(tc.M32 - 9, 20, **c)),
             (10.3, tc.tcp(0, 0, tc.ACK, rev=True, **a)),
             (11.0, tc.tcp(102, payload=b"LL", **a)), (11.1, tc.tcp(tc.M32 - 9 + 30, 20, **c)), (11.2, tc.tcp(104, payload=b"O", **a)),
             (11.3, tc.tcp(tc.M32 - 9 + 40, 20, **c)),
             (12.0, tc.tcp(700, 5, rev=True, **c)), (12.1, tc.tcp(705, 5, rev=True, **c)), (12.2, tc.tcp(700, 5, rev=True, **c))]
    fin = tmp_path / "idle.pcap"
    fin.write_bytes(pu.global_header() + b"".join(
        struct.pack("<IIII", 1_700_000_000 + int(t), round(t % 1 * 1_000_000), len(f), len(f)) + f for t, f in timed))
    names = ("seq_packets", "old_packets", "gap_packets", "overlap_packets", "old_bytes", "gap_bytes")
    got = {}
    for extra in (["--idle", "5"], []):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--bidirectional", "--track",
                            "--seq", "--chunk-packets", "4", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        rows = list(csv.DictReader(io.StringIO(r.stdout)))
        got[bool(extra)] = {int(x["sport"]): ([int(x[n]) for n in names], [int(x[n + "_rev"]) for n in names]) for x in rows}
        if extra:
            assert [int(x["sport"]) for x in rows] == [40002, 40001, 40003], "the idle connection is printed when it ages out"
    assert got[True] == got[False] == {40001: ([5, 1, 0, 0, 2, 0], [0] * 6), 40002: ([3, 1, 0, 0, 2, 0], [0] * 6),
                                       40003: ([3, 0, 1, 1, 10, 10], [3, 1, 0, 0, 5, 0])}


@pytest.mark.parametrize("chunk", [0, 4])
def test_skip_retransmits_reads_the_stream_once(tmp_path, chunk):
    """chunk = 4 puts the retransmit and its original into different device batches."""
    frames, conn = capture()
    extra = ["--chunk", str(chunk)] if chunk else []
    text, out = run_tool(tmp_path, "pcap_sessions.py", ["--stream", "HELLO", *extra])
    assert out == pu.build(frames, keep=[False] * len(frames)) and json.loads(text.strip().splitlines()[-1])["stream_hit_packets"] == 0
    text, out = run_tool(tmp_path, "pcap_sessions.py", ["--stream", "HELLO", "--skip-retransmits", *extra])
    res = json.loads(text.strip().splitlines()[-1])
    assert out == pu.build(frames, keep=[k == 0 for k in conn])
    assert res["stream_hit_packets"] == 1 and res["old_packets"] == 3 and res["seq_packets"] == 14 and res["marked_flows"] == 1
    text, out = run_tool(tmp_path, "pcap_sessions.py", ["--stream", "abab", *extra])
    assert out == pu.build(frames, keep=[k == 1 for k in conn])
    text, out = run_tool(tmp_path, "pcap_sessions.py", ["--stream", "abab", "--skip-retransmits", *extra])
    assert out == pu.build(frames, keep=[False] * len(frames))


@pytest.mark.parametrize("extra", [[], ["--chunk-packets", "4"], ["--stats"]])
def test_pcap_flows_prints_the_planted_counts(tmp_path, extra):
    text, _ = run_tool(tmp_path, "pcap_flows.py", ["--track", "--seq", *extra])
    rows = {int(r["sport"]): r for r in csv.DictReader(io.StringIO(text))}
    names = ("seq_packets", "old_packets", "gap_packets", "overlap_packets", "old_bytes", "gap_bytes")
    got = {sp: ([int(r[c]) for c in names], [int(r[c + "_rev"]) for c in names]) for sp, r in rows.items()}
    assert got[40001] == ([5, 1, 0, 0, 2, 0], [0, 0, 0, 0, 0, 0])     # SYN, HE, LL, LL again, O; the reply's pure ACK is no segment
    assert got[40002] == ([3, 1, 0, 0, 2, 0], [0, 0, 0, 0, 0, 0])     # SYN, ab, ab again
    assert got[40003] == ([3, 0, 1, 1, 10, 10], [3, 1, 0, 0, 5, 0])   # 10 bytes lost, then 10 of 20 bytes again, across the wrap
    plain, _ = run_tool(tmp_path, "pcap_flows.py", ["--track", *extra])
    width = len(plain.splitlines()[0].split(","))   # without the option the output is as before: the new columns come last
    assert "seq_packets" not in plain and [ln.split(",") for ln in plain.splitlines()] == [ln.split(",")[:width] for ln in text.splitlines()]

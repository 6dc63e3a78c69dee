"""GPU: tools/pcap_sessions.py --stream as a child process over a capture written here: three
connections, one whose request line is split over two TCP segments, one that holds it whole, one
without it. The stream matcher selects the first two whole, the per-packet PAYLOAD filter only the
second, and --invert writes the complement; a pattern the matcher refuses ends the tool by name."""
import json
import os
import subprocess
import sys

import pytest

import flowstream_cases as fc
import pcap_util as pu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def capture():
    """(frames, the connection of each: 0 split, 1 whole, 2 without)."""
    a, b, c = dict(sp=40001), dict(sp=40002), dict(sp=40003)
    ra, rb, rc = dict(dp=40001), dict(dp=40002), dict(dp=40003)
    rows = [(0, fc.frame(b"", **a)), (1, fc.frame(b"", **b)), (0, fc.frame(b"GE", **a)), (2, fc.frame(b"HELLO", **c)),
            (0, fc.frame(b"", src=fc.SERVER, dst=fc.CLIENT, sp=80, **ra)), (1, fc.frame(b"GET /index.html HTTP/1.1\r\n", **b)),
            (0, fc.frame(b"T / HTTP/1.1\r\nHost: a\r\n\r\n", **a)), (2, fc.frame(b"WORLD", src=fc.SERVER, dst=fc.CLIENT, sp=80, **rc)),
            (1, fc.frame(b"HTTP/1.1 200 OK\r\n", src=fc.SERVER, dst=fc.CLIENT, sp=80, **rb)),
            (0, fc.frame(b"HTTP/1.1 404\r\n", src=fc.SERVER, dst=fc.CLIENT, sp=80, **ra)), (2, fc.frame(b"GE", **c)), (2, fc.frame(b"x", **c))]
    return [f for _, f in rows], [k for k, _ in rows]


def run_tool(tmp_path, extra, ok=True):
    frames, _ = capture()
    fin, fout = tmp_path / "in.pcap", tmp_path / "out.pcap"
    fin.write_bytes(pu.build(frames))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_sessions.py"), "--in", str(fin), "--out", str(fout),
                        "--bidirectional", *extra], capture_output=True, text=True, timeout=120)
    if not ok:
        return r, fout
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), fout.read_bytes()


@pytest.mark.parametrize("chunk", [0, 3])
def test_stream_selects_the_split_request_too(tmp_path, chunk):
    """chunk = 3 puts the two halves of the split request into different device batches."""
    frames, conn = capture()
    extra = ["--chunk", str(chunk)] if chunk else []
    res, out = run_tool(tmp_path, ["--stream", "GET /", *extra])
    assert out == pu.build(frames, keep=[k in (0, 1) for k in conn])
    assert res["stream_hit_packets"] == 2 and res["marked_flows"] == 2 and res["flows"] == 3 and res["written_packets"] == 8
    res, out = run_tool(tmp_path, ["--filter", "payload:GET /", *extra])
    assert out == pu.build(frames, keep=[k == 1 for k in conn]) and "stream_hit_packets" not in res
    res, out = run_tool(tmp_path, ["--stream", "GET /", "--invert", *extra])
    assert out == pu.build(frames, keep=[k == 2 for k in conn]) and res["written_packets"] == 4
    res, out = run_tool(tmp_path, ["--stream", "GET /", "--filter", "payload:HELLO", *extra])
    assert out == pu.build(frames) and res["marked_flows"] == 3 and res["hit_packets"] == 1


def test_a_refused_pattern_ends_the_tool_by_name(tmp_path):
    for expr, word in (("GET.+", "repeatable"), ("^GET", "anchor"), ("(", "std::regex")):
        r, fout = run_tool(tmp_path, ["--stream", expr], ok=False)
        assert r.returncode != 0 and word in r.stderr and "--stream" in r.stderr and not fout.exists(), r.stderr

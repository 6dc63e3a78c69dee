"""GPU: tools/pcap_flows.py --track in a fresh child process: one flow tracker on the device for the
whole file must print what the default path (a download and a merge per chunk) prints, byte for
byte, stdout and the stderr totals alike; and --idle, whose expected lines come from the
restatement in flowtrack_ref.py."""
import csv
import io
import ipaddress
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import flowtab_ref as ftr
import flowtrack_ref as fkr
import pcap_util
from test_gpu_pcap_flows import NAMES, _tcp, _udp, _v4, conversations

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(fin, chunk, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--chunk-packets",
                        str(chunk), *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout, r.stderr


@pytest.mark.parametrize("extra", [[], ["--bidirectional"], ["--filter", "protocol:tcp"],
                                   ["--filter", "protocol:tcp", "--bidirectional", "--l3-only"],
                                   ["--bidirectional", "--format", "json", "--top", "3"]], ids=lambda e: " ".join(e) or "plain")
def test_track_prints_what_the_default_path_prints(tmp_path, extra):
    frames = conversations()
    fin = tmp_path / "conv.pcap"
    fin.write_bytes(pcap_util.build(frames))
    plain, tracked = _tool(fin, 50, extra), _tool(fin, 50, extra + ["--track"])
    assert tracked == plain
    assert json.loads(plain[1].strip().splitlines()[-1])["chunks"] == 4 and len(plain[0].splitlines()) > 2


def _pcap(frames, secs):
    """Microsecond pcap, record k at secs[k] seconds and k microseconds."""
    parts = [pcap_util.global_header()]
    for k, (f, t) in enumerate(zip(frames, secs)):
        parts.append(struct.pack("<IIII", t, k, len(f), len(f)) + f)
    return b"".join(parts)


def _lines(recs, starts):
    out = []
    for f in recs:
        k, key = int(f["klass"]), f["key"].tobytes()
        alen = 4 if k in (fr.V4, fr.V4_L4) else 16
        ports = k in (fr.V4_L4, fr.V6_L4)
        ts = [f"{int(f[c]) // 1000000}.{int(f[c]) % 1000000:06d}" for c in ("first_ts", "last_ts")]
        out.append({"class": NAMES[k], "src": str(ipaddress.ip_address(key[:alen])), "dst": str(ipaddress.ip_address(key[alen:2 * alen])),
                    "sport": str(int.from_bytes(key[2 * alen:2 * alen + 2], "big")) if ports else "",
                    "dport": str(int.from_bytes(key[2 * alen + 2:2 * alen + 4], "big")) if ports else "",
                    "packets": str(f["packets"][0]), "bytes": str(f["bytes"][0]), "packets_rev": str(f["packets"][1]),
                    "bytes_rev": str(f["bytes"][1]), "first": str(starts[f["first_batch"]] + f["first"]),
                    "last": str(starts[f["last_batch"]] + f["last"]), "first_ts": ts[0], "last_ts": ts[1]})
    return out


def test_idle_flows_age_out_chunk_by_chunk(tmp_path):
    """150 packets a second apart in chunks of 50, idle 40 s. Flow A speaks in the first chunk only
    and flow C in the first 30 packets and again in the last 30: both age out after the second
    chunk, and C comes back as a new line; flow B and the UDP flow D never pause."""
    a, b = [10, 0, 0, 1], [10, 0, 0, 2]
    frames = []
    for k in range(150):
        if k % 5 == 4:
            frames.append(_v4(b, a, 17, _udp(53, 5353, bytes(k % 9))))          # D
        elif k % 2 == 0 and k < 50:
            frames.append(_v4(a, b, 6, _tcp(1111, 80, bytes(k % 7))))           # A
        elif k % 3 == 0 and (k < 30 or k >= 120):
            frames.append(_v4(b, a, 6, _tcp(2222, 443, b"")))                   # C
        else:
            frames.append(_v4(a, b, 6, _tcp(3333, 22, bytes(3))) if k % 2 else _v4(b, a, 6, _tcp(22, 3333, bytes(5))))   # B
    secs = [5000 + k for k in range(150)]
    fin = tmp_path / "idle.pcap"
    fin.write_bytes(_pcap(frames, secs))
    ref = fkr.Tracker(150, ftr.BIDIRECTIONAL)
    inputs, nbytes, klass = fr.key_of_frames(frames)
    ts = np.array([s * 1000000 + k for k, s in enumerate(secs)], np.uint64)
    starts, want = [0, 50, 100], []
    for lo in starts:
        ref.update(inputs[lo:lo + 50], nbytes[lo:lo + 50], klass[lo:lo + 50], [len(f) for f in frames[lo:lo + 50]], None, ts[lo:lo + 50])
        want += _lines(ref.expire(int(ts[lo + 49]), 40 * 1000000, 150)["expired"], starts)
    aged = len(want)
    want += _lines(ref.records(), starts)
    assert aged == 2 and len(want) == 5 and want[0]["dport"] == "80" and want[1]["last"] == "27" and want[-1]["first"] == "120"
    out, err = _tool(fin, 50, ["--track", "--idle", "40", "--bidirectional"])
    got = list(csv.DictReader(io.StringIO(out)))
    assert got == want
    totals = json.loads(err.strip().splitlines()[-1])
    assert totals == {"packets": 150, "selected": 150, "no_key": 0, "chunks": 3, "truncated": 0, "flows": 5}
    # with an idle time nothing reaches, the lines are those of the plain --track path plus the two columns
    out2, _ = _tool(fin, 50, ["--track", "--idle", "1000", "--bidirectional"])
    base, _ = _tool(fin, 50, ["--track", "--bidirectional"])
    strip = [{k: v for k, v in r.items() if k not in ("first_ts", "last_ts")} for r in csv.DictReader(io.StringIO(out2))]
    assert strip == list(csv.DictReader(io.StringIO(base))) and len(strip) == 4

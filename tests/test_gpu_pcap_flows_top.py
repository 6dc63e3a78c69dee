"""GPU: tools/pcap_flows.py --track --top N takes the top from the device (bt_flow_track_top_device):
on a small crafted capture with deliberate byte-count ties the output is byte-equal to the default
path's, and --by syn orders the rows as the restatement (flowtop_ref.order over counts restated here
from the crafted packets) does."""
import csv
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import flowtcp_ref as tr
import flowtop_ref as top
import pcap_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "pcap_flows.py")
A, B = [10, 0, 0, 1], [10, 0, 0, 2]
CONVS = 12


def _tcp(src, dst, sp, dp, flags, pad):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, flags]) + bytes(6 + pad)


def packets():
    """(conversation, direction, flags, pad) per packet, conversations interleaved over several chunks.
    Conversations c and c + 6 carry the same bytes (a tie the earlier one wins); conversation c sends
    c % 4 SYNs, so the SYN counts tie as well."""
    p = []
    for rnd in range(5):
        for c in range(CONVS):
            if rnd < 1 + c % 6:   # 1 .. 6 packets of 60 + 10 (c % 3) bytes
                syn = rnd < c % 4
                p.append((c, rnd % 2 if not syn else 0, tr.SYN if syn else tr.ACK, 6 + 10 * (c % 3)))
    return p


def _frame(c, d, flags, pad):
    return _tcp(A, B, 1000 + c, 80, flags, pad) if d == 0 else _tcp(B, A, 80, 1000 + c, flags, pad)


def _run(fin, extra, ok=True):
    r = subprocess.run([sys.executable, TOOL, "--in", str(fin), "--chunk-packets", "14", "--bidirectional", *extra],
                       capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def test_top_from_the_device(tmp_path, gpu_ctx):
    pk = packets()
    fin = tmp_path / "top.pcap"
    fin.write_bytes(pcap_util.build([_frame(*p) for p in pk]))
    first = [next(i for i, p in enumerate(pk) if p[0] == c) for c in range(CONVS)]
    flow_of = sorted(range(CONVS), key=lambda c: first[c])   # flow number -> conversation: by first packet
    nbytes = np.array([sum(len(_frame(*p)) for p in pk if p[0] == c) for c in flow_of], np.uint64)
    syns = np.array([sum(1 for p in pk if p[0] == c and p[2] == tr.SYN) for c in flow_of], np.uint64)
    assert len(set(nbytes.tolist())) < CONVS and len(set(syns.tolist())) == 4   # ties in both measures

    # --by bytes (the default): byte-equal to the path that downloads every chunk's flows and sorts on the host
    want = _run(fin, ["--top", "5"])
    got = _run(fin, ["--track", "--top", "5"])
    assert got.stdout == want.stdout and got.stderr == want.stderr
    rows = list(csv.DictReader(io.StringIO(got.stdout)))
    assert [int(r["sport"]) - 1000 for r in rows] == [flow_of[f] for f in top.order(nbytes)[:5]]
    # the side table's columns beside the top
    both = list(csv.DictReader(io.StringIO(_run(fin, ["--track", "--tcp", "--top", "5"]).stdout)))
    assert [{k: r[k] for k in rows[0]} for r in both] == rows
    assert [int(r["syn"]) for r in both] == [int(syns[f]) for f in top.order(nbytes)[:5]]
    # N above 4096 keeps the host's sort
    assert _run(fin, ["--track", "--top", "5000"]).stdout == _run(fin, ["--top", "5000"]).stdout

    # --by syn: the non---track path has no such order; the rows against the restatement
    by_syn = list(csv.DictReader(io.StringIO(_run(fin, ["--track", "--tcp", "--top", "5", "--by", "syn"]).stdout)))
    order = top.order(syns)[:5]
    assert [int(r["sport"]) - 1000 for r in by_syn] == [flow_of[f] for f in order]
    assert [int(r["syn"]) for r in by_syn] == [int(syns[f]) for f in order] == [3, 3, 2, 2, 2]
    assert [int(r["bytes"]) + int(r["bytes_rev"]) for r in by_syn] == [int(nbytes[f]) for f in order]
    by_packets = list(csv.DictReader(io.StringIO(_run(fin, ["--track", "--top", "3", "--by", "packets"]).stdout)))
    npk = np.array([sum(1 for p in pk if p[0] == c) for c in flow_of], np.uint64)
    assert [int(r["sport"]) - 1000 for r in by_packets] == [flow_of[f] for f in top.order(npk)[:3]]

    assert "--by syn / rst: only with --tcp" in _run(fin, ["--track", "--top", "5", "--by", "syn"], ok=False).stderr
    assert "--by: only with --track and --top" in _run(fin, ["--top", "5", "--by", "packets"], ok=False).stderr
    assert "--by: only with --track and --top" in _run(fin, ["--track", "--top", "5000", "--by", "packets"], ok=False).stderr
    assert "no --top" in _run(fin, ["--track", "--idle", "5", "--top", "5"], ok=False).stderr

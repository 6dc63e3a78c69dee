"""GPU: tools/pcap_flows.py --track --tcp on a small crafted capture: the TCP columns against values
restated here from the crafted packets (flowtcp_ref's state function), and --closed-idle printing
closed and reset connections chunks before the others."""
import csv
import io
import json
import os
import subprocess
import sys

import pytest

import flowtcp_ref as tr
import pcap_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("none", "opening", "established", "closing", "closed", "reset", "midstream")
A, B = [10, 0, 0, 1], [10, 0, 0, 2]


def _tcp(src, dst, sp, dp, flags):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, flags]) + bytes(6)


def packets():
    """(conversation, direction, flags) per packet; pcap_util stamps packet k with second k // 7.
    Conversation 3 stays open through the whole file, 2 is half closed, 0 closes and 1 is reset in
    the first chunk of 14; 0 comes back in the last chunk."""
    S, K, F, R = tr.SYN, tr.ACK, tr.FIN, tr.RST
    p = [(3, 0, S), (3, 1, S | K), (2, 0, S), (2, 1, S | K), (2, 1, F | K),
         (0, 0, S), (0, 1, S | K), (0, 0, K), (0, 0, F | K), (0, 1, F | K), (1, 0, S), (1, 0, S), (1, 1, R | K), (3, 0, K)]
    p += [(3, k % 2, K | tr.PSH) for k in range(41)]
    return p + [(0, 0, S)]   # packet 55, second 7


def _frame(conv, d, flags):
    return _tcp(A, B, 1000 + conv, 80, flags) if d == 0 else _tcp(B, A, 80, 1000 + conv, flags)


def _expected(pk, lo=0):
    """The TCP columns and the counts of the packets pk (one conversation's), numbered from lo... by index."""
    fwd = rev = syn = fin = rst = 0
    for _, (conv, d, fl) in pk:
        fwd, rev = (fwd | fl, rev) if d == 0 else (fwd, rev | fl)
        syn += bool(fl & tr.SYN and not fl & tr.ACK)
        fin += bool(fl & tr.FIN)
        rst += bool(fl & tr.RST)
    conv = pk[0][1][0]
    return {"sport": str(1000 + conv), "packets": str(sum(1 for _, q in pk if q[1] == 0)), "packets_rev": str(sum(1 for _, q in pk if q[1] == 1)),
            "first": str(pk[0][0]), "last": str(pk[-1][0]), "tcp_flags_fwd": f"0x{fwd:02x}", "tcp_flags_rev": f"0x{rev:02x}",
            "tcp_state": NAMES[tr.state(fwd, rev, 2)], "syn": str(syn), "fin": str(fin), "rst": str(rst)}


def _run(fin, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--chunk-packets", "14",
                        "--bidirectional", "--track", *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return list(csv.DictReader(io.StringIO(r.stdout))), json.loads(r.stderr.strip().splitlines()[-1])


def _same(row, want):
    assert {k: row[k] for k in want} == want and row["src"] == "10.0.0.1" and row["dst"] == "10.0.0.2" and row["class"] == "ipv4_l4"


def test_tcp_columns_and_closed_idle(tmp_path, gpu_ctx):
    pk = packets()
    fin = tmp_path / "tcp.pcap"
    fin.write_bytes(pcap_util.build([_frame(*p) for p in pk]))
    by = {c: [(i, p) for i, p in enumerate(pk) if p[0] == c] for c in range(4)}
    # one wait, every flow at the end, in order of first packet: 3, 2, 0, 1
    rows, totals = _run(fin, ["--tcp"])
    assert totals["flows"] == 4 and totals["chunks"] == 4 and len(rows) == 4
    for row, c in zip(rows, (3, 2, 0, 1)):
        _same(row, _expected(by[c]))
    assert [r["tcp_state"] for r in rows] == ["established", "closing", "closed", "reset"]
    assert "first_ts" not in rows[0]
    # --idle alone: nothing is 100 s old, the same lines (with timestamps)
    idle, _ = _run(fin, ["--tcp", "--idle", "100"])
    assert [{k: v for k, v in r.items() if k not in ("first_ts", "last_ts")} for r in idle] == rows
    # --closed-idle 1: the closed and the reset conversation are printed after the second chunk (their last
    # packets are of second 1, the chunk's last of second 3), before the open ones; conversation 0's
    # last packet is a new flow, opening
    early, totals = _run(fin, ["--tcp", "--idle", "100", "--closed-idle", "1"])
    assert totals["flows"] == 5
    for row, want in zip(early, (_expected(by[0][:-1]), _expected(by[1]), _expected(by[3]), _expected(by[2]), _expected(by[0][-1:]))):
        _same(row, want)
    assert [r["tcp_state"] for r in early] == ["closed", "reset", "established", "closing", "opening"]
    # without the side table the tool prints what it always printed
    plain, _ = _run(fin, [])
    assert [dict(r) for r in plain] == [{k: v for k, v in r.items() if not k.startswith("tcp_") and k not in ("syn", "fin", "rst")} for r in rows]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--tcp"], capture_output=True, text=True)
    assert r.returncode != 0 and "--tcp: only with --track" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_flows.py"), "--in", str(fin), "--track", "--tcp", "--closed-idle", "1"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--closed-idle" in r.stderr

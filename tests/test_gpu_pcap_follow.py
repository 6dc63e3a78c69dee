"""GPU: tools/pcap_follow.py as a child process over a generated capture of two chunks: for a clean capture every
output file equals the generator's true stream of its direction; for a disturbed one the files equal what the
restatement in flowfollow_ref.py delivers chunk by chunk, and the printed bytes, runs and holes are the
restatement's, the holes also its table's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import flowfollow_ref as fr
import flowreasm_cases as rc
import pcap_util as pu
from beatrice_amd import abi
from test_flowstream import lay_out

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "pcap_follow.py")
BIDIR = 2


def name_of(frame):
    """tcpflow's name of the stream an Ethernet / IPv4 / TCP frame belongs to."""
    ip = lambda o: ".".join(f"{b:03d}" for b in frame[o:o + 4])  # noqa: E731
    port = lambda o: f"{int.from_bytes(frame[o:o + 2], 'big'):05d}"  # noqa: E731
    o4 = 14 + 4 * (frame[14] & 0xF)
    return f"{ip(26)}.{port(o4)}-{ip(30)}.{port(o4 + 2)}"


def two_chunks(seed, clean):
    """Two calls of flowreasm_cases.random_calls, the shorter filled up with UDP packets: (chunks, truth, the chunk size)."""
    calls, truth = rc.random_calls(seed, nflows=3, nbytes=900, ncalls=2, clean=clean)
    size = max(len(c) for c in calls)
    filler = [rc.other(rc.tcp(1, payload=b"filler", proto=17, sp=50000 + k), 0) for k in range(size)]
    return [c + filler[:size - len(c)] for c in calls], truth, size


def run_tool(tmp_path, chunks, size):
    fin, out = tmp_path / "in.pcap", tmp_path / "streams"
    fin.write_bytes(pu.build([r.frame for c in chunks for r in c]))
    r = subprocess.run([sys.executable, TOOL, "--in", str(fin), "--out-dir", str(out), "--bidirectional", "--chunk", str(size)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    printed = {}
    for ln in r.stdout.splitlines():
        name, *rest = ln.split()
        printed[name] = {k: int(v) for k, v in (x.split("=") for x in rest)}
    files = {p.name: p.read_bytes() for p in out.iterdir()}
    assert set(files) == set(printed)
    return files, printed


def test_a_clean_capture_gives_the_true_streams(tmp_path):
    chunks, truth, size = two_chunks(3, True)
    files, printed = run_tool(tmp_path, chunks, size)
    want = {}
    for key, s in truth.items():
        first = [r for c in chunks for r in c if r.key == key][0]
        want[name_of(first.frame)] = s
    assert files == want
    for key, s in truth.items():   # one run per chunk that holds a byte of the direction
        first = [r for c in chunks for r in c if r.key == key][0]
        runs = sum(any(r.key == key and r.data for r in c) for c in chunks)
        assert printed[name_of(first.frame)] == {"bytes": len(s), "runs": runs, "holes": 0}


def test_a_disturbed_capture_gives_the_restatements_runs(tmp_path):
    chunks, _, size = two_chunks(107, False)
    files, printed = run_tool(tmp_path, chunks, size)
    model = fr.Follow(3, None, BIDIR)
    seq_tab = np.zeros(3, abi.FlowTcpseqRec)
    want, counts, key_name = {}, {}, {}
    for rows in chunks:
        frames, ids = [r.frame for r in rows], np.array([r.flow if r.key is not None else 0xFFFFFFFD for r in rows], np.uint32)
        data, desc = lay_out(frames)
        off = np.full(len(rows), 7, np.int64)
        abi.flow_tcpseq_host(data, desc, ids, None, BIDIR, seq_tab, off=off)
        _, _, _, wbytes, wruns, wplace, _ = model.follow(frames, ids, off)
        for u in wruns:
            i = int(np.nonzero(wplace == u["at"])[0][0])   # the packet that delivered the run's first byte
            name = name_of(frames[i])
            key_name[(int(u["flow"]), int(u["flags"]) & 1)] = name
            want[name] = want.get(name, b"") + wbytes[int(u["at"]):int(u["at"] + u["len"])]
            c = counts.setdefault(name, {"bytes": 0, "runs": 0, "holes": 0})
            c["bytes"] += int(u["len"])
            c["runs"] += 1
            c["holes"] += bool(u["flags"] & fr.HOLE)
    assert files == want and printed == counts
    table = model.table
    assert {n: printed[n]["holes"] for n in printed} == {n: int(table[f]["d"][d]["holes"]) for (f, d), n in key_name.items()}
    assert sum(c["holes"] for c in counts.values()) >= 2

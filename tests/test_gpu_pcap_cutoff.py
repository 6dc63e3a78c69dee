"""GPU: tools/pcap_cutoff.py as a child process over pcaps built by pcap_util from the goldens. The
output must be, byte for byte, the pcap of the packets the restatement keeps (flowseq_ref.py over the
flow ids of flowtab_ref over the golden's records, the selection from the golden's code__<set>), and
the same for every chunk size. The limits are chosen so that this differs from both extremes."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import flowseq_ref as qr
import flowtab_ref as ftr
import pcap_util as pu
from beatrice_amd import abi
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {abi.BPF: "bpf", abi.PROTOCOL: "protocol", abi.IP_RANGE: "ip_range", abi.PORT_RANGE: "port_range", abi.PAYLOAD: "payload"}
FILTERS = {"http": "payload_re_11", "edge": "mixed"}
# capture: keyed packets, those of them --max-packets 3 keeps, unkeyed packets, packets of the largest flow (no filter, unidirectional)
FIRST_THREE = {"http": (2747, 2596, 253, 7), "edge": (197, 73, 122, 46)}


@functools.lru_cache(maxsize=None)
def expectation(cap, flags, filtered, mp, mb):
    """(filter arguments, frames, keep bits, the tool's JSON line) by the restatement."""
    g, man = load_golden(cap)
    n = len(g["desc"])
    args, sel = [], None
    if filtered:
        fset = FILTERS[cap]
        sel = fr.pack_bits(g[f"code__{fset}"] == 0)
        for f in man["filter_sets"][fset]:
            if not f.get("enabled", 1):   # a disabled filter takes no part; the tool has no switch for one
                continue
            assert not f.get("custom", 0)
            args += ["--filter", f"{NAMES[f['type']]}:{f.get('expr', '')}:{int(f.get('priority', 0))}"]
    keys = fr.key_of_rec(g["rec"], bool(flags & ftr.L3_ONLY))
    lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
    want = ftr.expected(*keys, lens, flags, sel)
    ids, nflows = want["flow_id"], want["result"]["n_flows"]
    table = np.zeros(nflows, qr.SEQ_REC)
    _, _, words, res = qr.number(table, ids, lens, sel, mp, mb, qr.KEEP_UNKEYED)
    keep = fr.select_bits(words, n).astype(bool)
    frames = pu.frames_of(g)
    line = {"packets": n, "selected": res["selected"], "flows": nflows, "numbered": res["numbered"], "unkeyed": res["unkeyed"],
            "written_packets": int(keep.sum()), "written_bytes": sum(len(f) for f, k in zip(frames, keep) if k)}
    assert res["bad_ids"] == 0 and res["kept"] == int(keep.sum())
    return args, frames, keep, line, int(table["packets"].max())


def run_tool(tmp_path, cap, flags, filtered, extra, ok=True):
    args, frames = expectation(cap, flags, filtered, 1, 0)[:2]
    fin, fout = tmp_path / "in.pcap", tmp_path / "out.pcap"
    fin.write_bytes(pu.build(frames))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_cutoff.py"), "--in", str(fin), "--out", str(fout), *args,
                        *(["--bidirectional"] if flags & ftr.BIDIRECTIONAL else []), *extra], capture_output=True, text=True, timeout=120)
    if not ok:
        return r, fout
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), fout.read_bytes()


def between(frames, keep, least):
    """The expectation lies strictly between the --max-packets 1 output and the whole capture."""
    assert (keep | least == keep).all() and int(least.sum()) < int(keep.sum()) < len(frames)


@pytest.mark.parametrize("flags", [0, ftr.BIDIRECTIONAL])
@pytest.mark.parametrize("chunk", [64, 256, 0])
@pytest.mark.parametrize("cap", sorted(FIRST_THREE))
def test_the_first_three_packets_of_every_flow_byte_for_byte(tmp_path, cap, chunk, flags):
    _, frames, keep, line, largest = expectation(cap, flags, False, 3, 0)
    between(frames, keep, expectation(cap, flags, False, 1, 0)[2])
    if not flags:
        keyed, kept, unkeyed, most = FIRST_THREE[cap]
        assert (line["numbered"], line["written_packets"] - line["unkeyed"], line["unkeyed"], largest) == (keyed, kept, unkeyed, most)
    res, out = run_tool(tmp_path, cap, flags, False, ["--max-packets", "3"] + (["--chunk", str(chunk)] if chunk else []))
    want = pu.build(frames, keep=keep)
    assert out == want, f"{cap} chunk={chunk} flags={flags}: {len(out)} bytes against {len(want)}"
    assert res == line


@pytest.mark.parametrize("flags", [0, ftr.BIDIRECTIONAL])
@pytest.mark.parametrize("cap", sorted(FILTERS))
def test_only_passing_packets_are_numbered(tmp_path, cap, flags):
    _, frames, keep, line, _ = expectation(cap, flags, True, 2, 0)
    g, _ = load_golden(cap)
    hit = g[f"code__{FILTERS[cap]}"] == 0
    assert (keep & ~hit).sum() == 0 and 0 < int(keep.sum()) < int(hit.sum()) == line["selected"] < len(frames)
    res, out = run_tool(tmp_path, cap, flags, True, ["--max-packets", "2", "--chunk", "256"])
    assert out == pu.build(frames, keep=keep) and res == line
    assert not (keep == expectation(cap, flags, False, 2, 0)[2]).all()   # numbering every packet keeps others


@pytest.mark.parametrize("flags", [0, ftr.BIDIRECTIONAL])
@pytest.mark.parametrize("cap,limit", [("http", 200), ("edge", 200)])
def test_a_byte_limit(tmp_path, cap, limit, flags):
    """The packet that crosses the limit is still written; the value lies between the extremes."""
    _, frames, keep, line, _ = expectation(cap, flags, False, 0, limit)
    between(frames, keep, expectation(cap, flags, False, 1, 0)[2])
    res, out = run_tool(tmp_path, cap, flags, False, ["--max-bytes", str(limit), "--chunk", "64"])
    assert out == pu.build(frames, keep=keep) and res == line
    both = expectation(cap, flags, False, 3, limit)
    res, out = run_tool(tmp_path, cap, flags, False, ["--max-bytes", str(limit), "--max-packets", "3"])
    assert out == pu.build(frames, keep=both[2]) and res == both[3]


def test_a_flow_cap_below_the_flows_leaves_no_output(tmp_path):
    _, frames, keep, line, _ = expectation("edge", 0, False, 3, 0)
    nflows = line["flows"]
    r, fout = run_tool(tmp_path, "edge", 0, False, ["--max-packets", "3", "--flow-cap", str(nflows - 1), "--chunk", "64"], ok=False)
    assert r.returncode != 0 and "--flow-cap" in r.stderr and not fout.exists()
    res, out = run_tool(tmp_path, "edge", 0, False, ["--max-packets", "3", "--flow-cap", str(nflows), "--chunk", "64"])
    assert res == line and out == pu.build(frames, keep=keep)


def test_a_limit_is_required(tmp_path):
    r, fout = run_tool(tmp_path, "edge", 0, False, [], ok=False)
    assert r.returncode != 0 and "--max-packets" in r.stderr and not fout.exists()

"""GPU: tools/pcap_sessions.py as a child process over pcaps built by pcap_util from the goldens. The
output must be, byte for byte, the pcap that keeps the records of every flow holding a packet the
reference passed (code__<set> == 0 of the golden; flows by flowtab_ref over the golden's records),
and the passing packets that have no flow key. The inputs are chosen so that this differs from the
plain filter's output and from the whole capture."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flow_ref as fr
import flowtab_ref as ftr
import pcap_util as pu
from beatrice_amd import abi
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {abi.BPF: "bpf", abi.PROTOCOL: "protocol", abi.IP_RANGE: "ip_range", abi.PORT_RANGE: "port_range", abi.PAYLOAD: "payload"}
# capture, filter set, packets, packets that pass, packets of a unidirectional flow with a passing packet
CASES = {"http": ("payload_re_11", 3000, 2476, 2531), "edge": ("mixed", 319, 100, 106)}


@functools.lru_cache(maxsize=None)
def expectation(cap, flags):
    """(filter arguments, frames, pass bits, session bits, flows, flows with a passing packet, passing packets without a key)."""
    fset = CASES[cap][0]
    g, man = load_golden(cap)
    hit = g[f"code__{fset}"] == 0
    keys = fr.key_of_rec(g["rec"], bool(flags & ftr.L3_ONLY))
    lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
    want = ftr.expected(*keys, lens, flags)
    ids, nflows = want["flow_id"], want["result"]["n_flows"]
    keyed = ids < nflows
    marked = np.zeros(nflows, bool)
    marked[ids[hit & keyed]] = True
    keep = hit.copy()
    keep[keyed] |= marked[ids[keyed]]
    args = []
    for f in man["filter_sets"][fset]:
        if not f.get("enabled", 1):   # a disabled filter takes no part; the tool has no switch for one
            continue
        assert not f.get("custom", 0)
        args += ["--filter", f"{NAMES[f['type']]}:{f.get('expr', '')}:{int(f.get('priority', 0))}"]
    return args, pu.frames_of(g), hit, keep, nflows, int(marked.sum()), int((hit & ~keyed).sum())


def run_tool(tmp_path, cap, flags, extra, ok=True):
    args, frames = expectation(cap, flags)[:2]
    fin, fout = tmp_path / "in.pcap", tmp_path / "out.pcap"
    fin.write_bytes(pu.build(frames))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_sessions.py"), "--in", str(fin), "--out", str(fout), *args,
                        *(["--bidirectional"] if flags & ftr.BIDIRECTIONAL else []), *(["--l3-only"] if flags & ftr.L3_ONLY else []), *extra], capture_output=True, text=True, timeout=120)
    if not ok:
        return r, fout
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), fout.read_bytes()


@pytest.mark.parametrize("flags", [0, ftr.BIDIRECTIONAL])
@pytest.mark.parametrize("chunk", [64, 256, 0])
@pytest.mark.parametrize("cap", sorted(CASES))
def test_whole_sessions_byte_for_byte(tmp_path, cap, chunk, flags):
    _, npk, npass, nsess = CASES[cap]
    _, frames, hit, keep, nflows, nmarked, unkeyed = expectation(cap, flags)
    # the expectation is neither the plain filter's output nor the whole capture
    assert len(frames) == npk and int(hit.sum()) == npass and npass < int(keep.sum()) < npk
    if not flags:
        assert int(keep.sum()) == nsess
    res, out = run_tool(tmp_path, cap, flags, ["--chunk", str(chunk)] if chunk else [])
    want = pu.build(frames, keep=keep)
    assert out == want, f"{cap} chunk={chunk} flags={flags}: {len(out)} bytes against {len(want)}"
    assert out != pu.build(frames, keep=hit) and out != pu.build(frames)
    assert res == {"packets": npk, "hit_packets": npass, "flows": nflows, "marked_flows": nmarked, "unkeyed_hits": unkeyed,
                   "written_packets": int(keep.sum()), "written_bytes": sum(len(f) for f, k in zip(frames, keep) if k)}


@pytest.mark.parametrize("cap,chunk", [("http", 256), ("edge", 64)])
def test_invert_writes_exactly_the_complement(tmp_path, cap, chunk):
    """With --l3-only a session is a pair of addresses: more packets belong to one, fewer are left."""
    flags = ftr.BIDIRECTIONAL | ftr.L3_ONLY
    _, frames, hit, keep, nflows, nmarked, unkeyed = expectation(cap, flags)
    assert int(keep.sum()) > CASES[cap][3]
    res, out = run_tool(tmp_path, cap, flags, ["--invert", "--chunk", str(chunk)])
    assert out == pu.build(frames, keep=~keep)
    assert res["written_packets"] == len(frames) - int(keep.sum()) > 0 and res["marked_flows"] == nmarked and res["hit_packets"] == int(hit.sum())


def test_a_flow_cap_below_the_flows_writes_nothing(tmp_path):
    nflows = expectation("edge", 0)[4]
    r, fout = run_tool(tmp_path, "edge", 0, ["--flow-cap", str(nflows - 1), "--chunk", "64"], ok=False)
    assert r.returncode != 0 and "--flow-cap" in r.stderr and not fout.exists()
    res, out = run_tool(tmp_path, "edge", 0, ["--flow-cap", str(nflows), "--chunk", "64"])
    assert res["flows"] == nflows and out == pu.build(expectation("edge", 0)[1], keep=expectation("edge", 0)[3])

"""GPU: tools/pcap_stats.py in a fresh child process over golden captures written as pcap files,
in chunks of 1,000 packets (several chunks: the BT_TALLY_ACCUMULATE path). Every number of its
JSON line is compared with numpy over the goldens' reference outcomes (code__* / src__*), records
and descriptor lengths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pcap_util
from conftest import load_golden
from golden_util import eval_order

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "bpf", 1: "protocol", 2: "ip_range", 3: "port_range", 4: "payload"}
LAYERS = {"ethernet": (0,), "vlan": (1, 2), "ipv4": (3,), "ipv6": (4,), "tcp": (5,), "udp": (6,), "icmp": (7,)}
CHUNK = 1000


def _expected(g, filters, fset):
    code, src = g[f"code__{fset}"], g[f"src__{fset}"]
    lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
    n = len(code)
    groups = {"passed": code == 0, "dropped": code == 1, "threw": code >= 2, "host": np.zeros(n, bool)}
    want = {"packets": n, "bytes": int(lens.sum()), "chunks": (n + CHUNK - 1) // CHUNK, "truncated": 0}
    for k, m in groups.items():
        want[k] = {"packets": int(m.sum()), "bytes": int(lens[m].sum())}
    counts = {}
    for i in eval_order(filters):   # the deciding filter of every decided packet, in evaluation order
        c = int(((code < 2) & (src == i)).sum())
        if c:
            key = f"{NAMES[filters[i]['type']]}:{filters[i]['expr']}"
            counts[key] = counts.get(key, 0) + c
    want["filter_counts"] = counts
    present, ok = g["rec"][:, 24], g["rec"][:, 25]
    want["layers"] = {}
    for name, bits in LAYERS.items():
        p = sum(int(((present >> b) & 1).sum()) for b in bits)
        o = sum(int(((ok >> b) & 1).sum()) for b in bits)
        want["layers"][name] = {"parsed": o, "failed": p - o}
    return want


@pytest.mark.parametrize("cap", ["fuzz", "c3"])
@pytest.mark.parametrize("fset", ["c3", "throw_after"])
def test_pcap_stats_tool(tmp_path, manifest, cap, fset):
    g, _ = load_golden(cap)
    filters = manifest["filter_sets"][fset]
    fin = tmp_path / f"{cap}.pcap"
    fin.write_bytes(pcap_util.build(pcap_util.frames_of(g)))
    args = []
    for f in filters:
        assert f.get("enabled", 1) and not f.get("custom", 0)
        args += ["--filter", f"{NAMES[f['type']]}:{f.get('expr', '')}:{int(f.get('priority', 0))}"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pcap_stats.py"), "--in", str(fin),
                        "--chunk-packets", str(CHUNK), *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = _expected(g, filters, fset)
    assert want["chunks"] > 1 and want["passed"]["packets"] + want["dropped"]["packets"] + want["threw"]["packets"] \
        == want["packets"]
    assert got == want, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
    assert list(got["filter_counts"]) == list(want["filter_counts"])   # evaluation order

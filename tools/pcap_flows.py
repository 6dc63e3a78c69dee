"""List the flows of a classic pcap capture from the GPU's flow table: one line per flow with its
class, addresses, ports, packets and bytes per direction, and the first and last packet number in
the file (the NetFlow / conntrack view of a capture).

Usage: python tools/pcap_flows.py --in a.pcap [--filter TYPE:EXPR[:PRIO] ...] [--bidirectional] [--l3-only]
                                  [--top N] [--format csv|json] [--chunk-packets N]
  --filter         as tools/pcap_filter.py takes it; only passing packets are counted
  --bidirectional  both directions of a conversation are one flow (BT_FLOWTAB_BIDIRECTIONAL): the
                   listed source is the smaller endpoint, packets_rev / bytes_rev count the other direction
  --l3-only        never key on ports (BT_FLOWTAB_L3_ONLY)
  --top N          the N flows with the most bytes, largest first (default: every flow, by first packet)
  --format         csv (default, with a header line) or json (one object per line)
  --chunk-packets  packets per device batch (default: at most 64 MiB of the file and 1M packets)
The file is taken in chunks of whole records, as tools/pcap_stats.py takes it. Per chunk: with
filters the filter-only bt_parse_filter_device, then bt_flow_table_device over its verdict words
(without filters over every packet). Only the 72-byte result and flows[0 .. n_written) come back
from the device; the chunks' flow lists are merged here by class and key. A program with a slot the
GPU cannot decide (BT_K_HOST) is refused. Packets without a flow key (not IP) are in no flow; their
count goes to stderr with the totals.
"""
from __future__ import annotations

import argparse
import ipaddress
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from beatrice_amd import abi  # noqa: E402
from pcap_filter import parse_filter  # noqa: E402
from pcap_stats import MASK48, chunks_of  # noqa: E402

K_HOST = 9   # enum bt_filter_kind
COLUMNS = ("class", "src", "dst", "sport", "dport", "packets", "bytes", "packets_rev", "bytes_rev", "first", "last")


def describe(klass: int, key: bytes, v: list) -> dict:
    """One output line: v = [packets, packets_rev, bytes, bytes_rev, first, last]."""
    alen = 4 if klass in (abi.FLOW_V4, abi.FLOW_V4_L4) else 16
    ports = klass in (abi.FLOW_V4_L4, abi.FLOW_V6_L4)
    p = key[2 * alen:2 * alen + 4]
    return {"class": abi.FLOW_NAMES[klass], "src": str(ipaddress.ip_address(key[:alen])),
            "dst": str(ipaddress.ip_address(key[alen:2 * alen])),
            "sport": int.from_bytes(p[0:2], "big") if ports else None, "dport": int.from_bytes(p[2:4], "big") if ports else None,
            "packets": v[0], "bytes": v[2], "packets_rev": v[1], "bytes_rev": v[3], "first": v[4], "last": v[5]}


def merge(table: dict, flows: np.ndarray, lo: int):
    """Add one chunk's records (packet numbers relative to `lo`) to the file's table."""
    for f in flows:
        k = (int(f["klass"]), f["key"].tobytes())
        p, b = f["packets"], f["bytes"]
        v = table.get(k)
        if v is None:
            table[k] = [int(p[0]), int(p[1]), int(b[0]), int(b[1]), lo + int(f["first"]), lo + int(f["last"])]
        else:
            v[0] += int(p[0]); v[1] += int(p[1]); v[2] += int(b[0]); v[3] += int(b[1])   # noqa: E702
            v[5] = lo + int(f["last"])   # chunks ascend


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--bidirectional", action="store_true")
    ap.add_argument("--l3-only", action="store_true")
    ap.add_argument("--top", type=int, default=0)
    ap.add_argument("--format", choices=("csv", "json"), default="csv")
    ap.add_argument("--chunk-packets", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.chunk_packets < 0 or a.top < 0:
        raise SystemExit("--chunk-packets / --top: want a positive count")
    filters = [parse_filter(f) for f in a.filter]
    data = np.fromfile(a.src, np.uint8)
    try:
        info, desc = abi.pcap_index(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_flows: {e}")
    flags = (abi.FLOWTAB_BIDIRECTIONAL if a.bidirectional else 0) | (abi.FLOWTAB_L3_ONLY if a.l3_only else 0)
    off, ln = (desc & MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    parts = list(chunks_of(off, ln, a.chunk_packets))
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) for lo, hi in parts), default=1)
    table: dict = {}
    totals = {"packets": int(len(desc)), "selected": 0, "no_key": 0, "chunks": len(parts), "truncated": info["truncated"]}
    ctx = abi.Context(a.device)
    try:
        if any(s.kind == K_HOST for s in ctx.compile(filters)):
            raise SystemExit("pcap_flows: a filter the GPU cannot decide (a CUSTOM callback, a PAYLOAD regex outside "
                             "its subset) is in the program")
        need = abi.flow_table_scratch_bytes(max_n, 0)
        d_data = ctx.alloc((max_bytes + 255) // 256 * 256 + 256)
        d_desc, d_ver = ctx.alloc(max(16, max_n * 8)), ctx.alloc(max(16, (max_n + 63) // 64 * 8))
        d_scratch, d_flows, d_res = ctx.alloc(need), ctx.alloc(80 * max_n), ctx.alloc(abi.ctypes.sizeof(abi.FlowTableResult))
        ctx.reserve(max_n)
        for lo, hi in parts:
            n, first = hi - lo, int(off[lo])
            nbytes = int(off[hi - 1] + ln[hi - 1]) - first
            d_data.upload(data[first:first + nbytes])   # waits for the context's stream: the last chunk is done
            d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
            batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, max(nbytes, 1), abi.DESC_PACKED, 0)
            if filters:
                ctx.run_device(batch, abi.Outputs(None, 0, d_ver.ptr, None, None, None))
            ctx.flow_table_device(batch, abi.FlowTableOpts(flags, 0, n, 0), d_scratch, need, d_res,
                                  select=d_ver if filters else None, flows=d_flows)
            ctx.synchronize()
            res = abi.FlowTableResult.from_bytes(d_res.download(np.zeros(d_res.nbytes, np.uint8))).as_dict()
            if res["overflow_packets"]:   # 2 n slots hold any n flows
                raise SystemExit("pcap_flows: the flow table overflowed")
            got = d_flows.download(np.zeros(80 * res["n_written"], np.uint8)) if res["n_written"] else np.zeros(0, np.uint8)
            merge(table, got.view(abi.FlowRec), lo)   # only the records cross PCIe
            totals["selected"] += res["n_selected"]
            totals["no_key"] += res["none_packets"]
        for b in (d_data, d_desc, d_ver, d_scratch, d_flows, d_res):
            b.free()
    except abi.BtError as e:
        raise SystemExit(f"pcap_flows: {e}")
    finally:
        ctx.close()
    rows = [describe(k[0], k[1], v) for k, v in table.items()]   # insertion order: by first packet
    if a.top:
        rows = sorted(rows, key=lambda r: (-(r["bytes"] + r["bytes_rev"]), r["first"]))[:a.top]
    if a.format == "csv":
        print(",".join(COLUMNS))
        for r in rows:
            print(",".join("" if r[c] is None else str(r[c]) for c in COLUMNS))
    else:
        for r in rows:
            print(json.dumps(r))
    totals["flows"] = len(table)
    print(json.dumps(totals), file=sys.stderr)


if __name__ == "__main__":
    main()

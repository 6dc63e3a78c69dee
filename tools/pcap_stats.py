"""Count a classic pcap capture on the GPU: packets and bytes by filter outcome, the reference's
filterCounts view, and the parsed layers, without a per-packet output ever leaving the device
(bt_parse_filter_device + bt_tally_device with BT_TALLY_ACCUMULATE). The counting twin of
tools/pcap_filter.py.

Usage: python tools/pcap_stats.py --in a.pcap [--filter TYPE:EXPR[:PRIO] ...] [--chunk-packets N]
  --filter         as tools/pcap_filter.py takes it
  --chunk-packets  packets per device batch (default: at most 64 MiB of the file and 1M packets)
The file is taken in chunks of whole records; every chunk is parsed and filtered on the device and
added to one bt_tally there, whose 2,304 bytes are copied back once, at the end. Prints one JSON
line:
  packets, bytes, chunks, truncated
  passed / dropped / threw / host   {"packets", "bytes"} by outcome (host: left to the host, a
                   PAYLOAD regex outside the GPU subset)
  filter_counts    PacketFilter::getStats().filterCounts for the decided packets: passes under
                   the last filter evaluated, rejects under the rejecting filter, keyed TYPE:EXPR
                   in evaluation order ("" with no filter)
  layers           per layer name, {"parsed", "failed"}: packets whose layer parsed / was
                   attempted and did not (vlan: both tags)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from beatrice_amd import abi  # noqa: E402
from pcap_filter import TYPES, parse_filter  # noqa: E402

MAX_CHUNK_BYTES = 64 << 20
MAX_CHUNK_PACKETS = 1 << 20
MASK48 = np.uint64((1 << 48) - 1)
LAYERS = {"ethernet": (0,), "vlan": (1, 2), "ipv4": (3,), "ipv6": (4,), "tcp": (5,), "udp": (6,), "icmp": (7,)}
TYPE_NAMES = {v: k for k, v in TYPES.items()}


def chunks_of(off: np.ndarray, ln: np.ndarray, chunk_packets: int):
    """[lo, hi) packet ranges of whole records: chunk_packets each when given, else as many as
    span at most 64 MiB of the file and 1M packets (at least one)."""
    n, lo = len(off), 0
    end = off + ln
    while lo < n:
        if chunk_packets:
            hi = min(n, lo + chunk_packets)
        else:
            hi = int(np.searchsorted(end, off[lo] + MAX_CHUNK_BYTES, side="right"))
            hi = max(lo + 1, min(hi, lo + MAX_CHUNK_PACKETS, n))
        yield lo, hi
        lo = hi


def report(t: dict, filters: list, order: list, chunks: int, truncated: int) -> dict:
    """The JSON line from the tally's dict; order[s] = the index in `filters` of program slot s."""
    names = ["pass", "reject", "throw", "host"]
    by = {k: {"packets": t["code"][c], "bytes": t["bytes"][c]} for c, k in enumerate(names)}
    keys = [f"{TYPE_NAMES[filters[i]['type']]}:{filters[i]['expr']}" for i in order]
    counts: dict = {}
    if not keys:
        if t["code"][0] + t["code"][1]:
            counts[""] = t["code"][0] + t["code"][1]
    else:
        for s, k in enumerate(keys):
            c = t["slot"][abi.DECIDE_REJECT][s] + (t["code"][abi.DECIDE_PASS] if s == len(keys) - 1 else 0)
            if c:
                counts[k] = counts.get(k, 0) + c
    layers = {}
    for name, bits in LAYERS.items():
        ok = sum(t["layer_ok"][b] for b in bits)
        layers[name] = {"parsed": ok, "failed": sum(t["layer_present"][b] for b in bits) - ok}
    return {"packets": t["n"], "bytes": sum(t["bytes"]), "chunks": chunks, "truncated": truncated,
            "passed": by["pass"], "dropped": by["reject"], "threw": by["throw"], "host": by["host"],
            "filter_counts": counts, "layers": layers}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--chunk-packets", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.chunk_packets < 0:
        raise SystemExit("--chunk-packets: want a positive count")
    filters = [parse_filter(f) for f in a.filter]
    data = np.fromfile(a.src, np.uint8)
    try:
        info, desc = abi.pcap_index(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_stats: {e}")
    off, ln = (desc & MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    parts = list(chunks_of(off, ln, a.chunk_packets))
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) for lo, hi in parts), default=1)
    ctx = abi.Context(a.device)
    try:
        order = [s.source_index for s in ctx.compile(filters)]
        d_data = ctx.alloc((max_bytes + 255) // 256 * 256 + 256)
        d_desc, d_dec = ctx.alloc(max(16, max_n * 8)), ctx.alloc(max(16, max_n))
        d_rec, d_tally = ctx.alloc((max_n + 63) // 64 * 6144), ctx.alloc(abi.ctypes.sizeof(abi.Tally))
        ctx.reserve(max_n)
        d_tally.zero()
        for lo, hi in parts:
            n, first = hi - lo, int(off[lo])
            nbytes = int(off[hi - 1] + ln[hi - 1]) - first
            d_data.upload(data[first:first + nbytes])   # waits for the context's stream: the last chunk is done
            d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
            batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, max(nbytes, 1), abi.DESC_PACKED, 0)
            ctx.run_device(batch, abi.Outputs(d_rec.ptr, n, None, d_dec.ptr, None, None))
            ctx.tally_device(d_dec, n, d_tally, frames=batch, records_ptr=d_rec, n_cap=n, flags=abi.TALLY_ACCUMULATE)
        ctx.synchronize()
        tally = abi.Tally.from_bytes(d_tally.download(np.zeros(d_tally.nbytes, np.uint8))).as_dict()
        for b in (d_data, d_desc, d_dec, d_rec, d_tally):
            b.free()
    except abi.BtError as e:
        raise SystemExit(f"pcap_stats: {e}")
    finally:
        ctx.close()
    print(json.dumps(report(tally, filters, order, len(parts), info["truncated"])))


if __name__ == "__main__":
    main()

"""Fan a classic pcap capture out to K files by RSS flow hash on the GPU: P.q.pcap holds the
input's global header and the passing records of queue q, verbatim and in capture order, so a
flow's packets stay in one file (with --symmetric, both directions of a connection).

Usage: python tools/pcap_fanout.py --in a.pcap --queues K --out-prefix P [--filter TYPE:EXPR[:PRIO] ...]
                                   [--symmetric] [--l3-only] [--chunk-packets N]
  --filter         as tools/pcap_filter.py takes it; only passing packets are fanned out
  --symmetric      the 0x6d5a-repeated key (BT_FANOUT_KEY_SYMMETRIC) instead of the RSS verification key
  --l3-only        never hash ports (BT_FANOUT_L3_ONLY)
  --chunk-packets  packets per device batch (default: at most 64 MiB of the file and 1M packets)
The file is taken in chunks of whole records, as tools/pcap_stats.py takes it. Per chunk: the
filter-only bt_parse_filter_device, bt_flow_fanout_device over its verdict words, then one
bt_pass_pack_device (lead 16: the record header goes along) per non-empty queue over that queue's
row of select_q, sized from result.bytes[q] + 16 * count. Only the 808-byte result and the packed
bytes come back from the device. A program with a slot the GPU cannot decide (BT_K_HOST) is refused.
Prints one JSON line: packets, passed, chunks, truncated, per-queue packets and bytes (frame
bytes, without the record headers), and the passing packets by flow class.
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
from pcap_filter import parse_filter  # noqa: E402
from pcap_stats import MASK48, chunks_of  # noqa: E402

K_HOST = 9   # enum bt_filter_kind
LEAD = 16    # a pcap record header


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True)
    ap.add_argument("--queues", type=int, required=True)
    ap.add_argument("--out-prefix", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--symmetric", action="store_true")
    ap.add_argument("--l3-only", action="store_true")
    ap.add_argument("--chunk-packets", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if not 1 <= a.queues <= abi.FANOUT_MAX_QUEUES:
        raise SystemExit(f"--queues: want 1..{abi.FANOUT_MAX_QUEUES}")
    if a.chunk_packets < 0:
        raise SystemExit("--chunk-packets: want a positive count")
    filters = [parse_filter(f) for f in a.filter]
    data = np.fromfile(a.src, np.uint8)
    try:
        info, desc = abi.pcap_index(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_fanout: {e}")
    K = a.queues
    opts = abi.FanoutOpts.make(K, (abi.FANOUT_KEY_SYMMETRIC if a.symmetric else 0) | (abi.FANOUT_L3_ONLY if a.l3_only else 0))
    off, ln = (desc & MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    parts = list(chunks_of(off, ln, a.chunk_packets))
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) + LEAD for lo, hi in parts), default=1)
    packets, nbytes, klass, passed = [0] * K, [0] * K, [0] * 5, 0
    ctx = abi.Context(a.device)
    outs = [open(f"{a.out_prefix}.{q}.pcap", "wb") for q in range(K)]
    try:
        if any(s.kind == K_HOST for s in ctx.compile(filters)):
            raise SystemExit("pcap_fanout: a filter the GPU cannot decide (a CUSTOM callback, a PAYLOAD regex outside "
                             "its subset) is in the program")
        for fh in outs:
            fh.write(data[:24].tobytes())
        tiles = (max_n + 63) // 64
        d_data = ctx.alloc((max_bytes + 255) // 256 * 256 + 256)
        d_desc, d_ver = ctx.alloc(max(16, max_n * 8)), ctx.alloc(max(16, tiles * 8))
        d_rows, d_res = ctx.alloc(max(16, K * tiles * 8)), ctx.alloc(abi.ctypes.sizeof(abi.FanoutResult))
        d_pack, d_tot, d_np = ctx.alloc(max_bytes + LEAD * max_n + 256), ctx.alloc(8), ctx.alloc(8)
        ctx.reserve(max_n)
        for lo, hi in parts:
            n = hi - lo
            first = int(off[lo]) - LEAD   # the chunk starts at its first record's header
            size = int(off[hi - 1] + ln[hi - 1]) - first
            d_data.upload(data[first:first + size])   # waits for the context's stream: the last chunk is done
            d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
            batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, size, abi.DESC_PACKED, 0)
            ctx.run_device(batch, abi.Outputs(None, 0, d_ver.ptr, None, None, None))
            ctx.flow_fanout_device(batch, opts, d_res, select=d_ver, select_q=d_rows)
            ctx.synchronize()
            res = abi.FanoutResult.from_bytes(d_res.download(np.zeros(d_res.nbytes, np.uint8))).as_dict()
            passed += res["n_selected"]
            klass = [x + y for x, y in zip(klass, res["klass"])]
            rows = (n + 63) // 64
            for q in range(K):
                count = res["start"][q + 1] - res["start"][q]
                if not count:
                    continue
                need = res["bytes"][q] + LEAD * count
                ctx.pass_pack(batch, d_rows.ptr + 8 * q * rows, d_pack, need, d_tot, d_np, lead=LEAD)
                ctx.synchronize()
                got = d_pack.download(np.zeros(need, np.uint8))   # only the packed bytes cross PCIe
                if int(d_tot.download(np.zeros(1, np.uint64))[0]) != need or \
                        int(d_np.download(np.zeros(2, np.uint32))[0]) != count:
                    raise SystemExit(f"pcap_fanout: queue {q}: the pack disagrees with the fan-out's sizes")
                outs[q].write(got.tobytes())
                packets[q] += count
                nbytes[q] += res["bytes"][q]
        for b in (d_data, d_desc, d_ver, d_rows, d_res, d_pack, d_tot, d_np):
            b.free()
    except abi.BtError as e:
        raise SystemExit(f"pcap_fanout: {e}")
    finally:
        for fh in outs:
            fh.close()
        ctx.close()
    print(json.dumps({"packets": int(len(desc)), "passed": passed, "chunks": len(parts), "truncated": info["truncated"],
                      "queues": [{"packets": p, "bytes": b} for p, b in zip(packets, nbytes)],
                      "classes": dict(zip(abi.FLOW_NAMES, klass))}))


if __name__ == "__main__":
    main()

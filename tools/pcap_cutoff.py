"""Write the first K packets / the first B bytes of every connection of a capture (of the packets
that pass the filters, when filters are given): the per-flow cut-off, decided on the GPU.

Usage: python tools/pcap_cutoff.py --in a.pcap --out b.pcap [--filter TYPE:EXPR[:PRIO] ...]
                                   [--bidirectional] [--l3-only] --max-packets K --max-bytes B
                                   [--flow-cap N] [--chunk PACKETS]
  --filter         as tools/pcap_filter.py takes it; only passing packets are numbered
  --bidirectional  both directions of a conversation are one flow (BT_FLOWTAB_BIDIRECTIONAL)
  --l3-only        never key on ports (BT_FLOWTAB_L3_ONLY): a flow is a pair of addresses
  --max-packets K  keep a packet while fewer than K packets of its flow came before it
  --max-bytes B    ... and fewer than B bytes: the packet that crosses B is kept, the next is not
                   (at least one of the two limits; 0 = no limit)
  --flow-cap N     room for N flows in the tracker (default: one per packet of the file)
  --chunk PACKETS  packets per device batch (default: at most 64 MiB of the file and 1M packets)
The file is taken in chunks of whole records, as tools/pcap_stats.py takes it, once: a cut-off is
causal, a packet's fate depends only on what came before it. Per chunk: the filter-only
bt_parse_filter_device when filters are given (its verdict is the selection, else every packet),
bt_flow_track_update_device over the selected packets (one tracker for the whole file, so a flow
keeps its number from chunk to chunk), bt_flow_seq_device with BT_FLOW_SEQ_KEEP_UNKEYED against one
sequence table for the file (a selected packet without a flow key is a flow of its own, as in
tools/pcap_sessions.py), then bt_pass_pack_device with lead 16, so that the record headers go along.
Only the packed bytes come back. The output records are verbatim and in order behind the input's
global header. The tracker's header is read at the end: more flows than --flow-cap remove the output
and end the run non-zero. A program with a slot the GPU cannot decide (BT_K_HOST) is refused.
Prints one JSON line: packets, selected, flows, numbered, unkeyed, written_packets, written_bytes.
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
    ap.add_argument("--out", dest="dst", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--bidirectional", action="store_true")
    ap.add_argument("--l3-only", action="store_true")
    ap.add_argument("--max-packets", type=int, default=0, metavar="K")
    ap.add_argument("--max-bytes", type=int, default=0, metavar="B")
    ap.add_argument("--flow-cap", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0, metavar="PACKETS")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.chunk < 0 or a.flow_cap < 0 or a.max_packets < 0 or a.max_bytes < 0:
        raise SystemExit("--chunk / --flow-cap / --max-packets / --max-bytes: want a positive count")
    if not a.max_packets and not a.max_bytes:
        raise SystemExit("--max-packets / --max-bytes: want at least one limit (without one every packet is kept: copy the file)")
    filters = [parse_filter(f) for f in a.filter]
    data = np.fromfile(a.src, np.uint8)
    try:
        info, desc = abi.pcap_index(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_cutoff: {e}")
    flags = (abi.FLOWTAB_BIDIRECTIONAL if a.bidirectional else 0) | (abi.FLOWTAB_L3_ONLY if a.l3_only else 0)
    off, ln = (desc & MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    parts = list(chunks_of(off, ln, a.chunk))
    total_n = len(off)
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) + LEAD for lo, hi in parts), default=1)
    cap = a.flow_cap or max(1, total_n)
    out = {"packets": total_n, "selected": 0, "flows": 0, "numbered": 0, "unkeyed": 0, "written_packets": 0, "written_bytes": 0}
    ctx = abi.Context(a.device)
    fh, whole = None, False
    try:
        if filters and any(s.kind == K_HOST for s in ctx.compile(filters)):
            raise SystemExit("pcap_cutoff: a filter the GPU cannot decide (a CUSTOM callback, a PAYLOAD regex outside "
                             "its subset) is in the program")
        lay = abi.flow_track_layout(cap)
        need = abi.flow_track_scratch_bytes(max_n)
        seq_need = abi.flow_seq_scratch_bytes(max_n, cap)
        d_state, d_scratch, d_res = ctx.alloc(lay["total"]), ctx.alloc(need), ctx.alloc(64)
        d_seq_tab, d_seq_scratch, d_seq_res = ctx.alloc(16 * cap), ctx.alloc(max(256, seq_need)), ctx.alloc(64)
        d_ids, d_ver = ctx.alloc(max(16, 4 * max_n)), ctx.alloc(max(16, (max_n + 63) // 64 * 8))
        d_data = ctx.alloc((max_bytes + 255) // 256 * 256 + 256)
        d_desc = ctx.alloc(max(16, max_n * 8))
        d_sel = ctx.alloc(max(16, (max_n + 63) // 64 * 8))
        d_pack, d_tot, d_np = ctx.alloc(max_bytes + LEAD * max_n + 256), ctx.alloc(8), ctx.alloc(8)
        bufs = [d_state, d_scratch, d_res, d_seq_tab, d_seq_scratch, d_seq_res, d_ids, d_ver, d_data, d_desc, d_sel, d_pack, d_tot, d_np]
        d_seq_tab.zero()
        ctx.reserve(max_n)
        ctx.flow_track_init(d_state, lay["total"], cap, flags)
        fh = open(a.dst, "wb")
        fh.write(data[:24].tobytes())
        for lo, hi in parts:
            n = hi - lo
            first = int(off[lo]) - LEAD   # the chunk starts at its first record's header
            size = int(off[hi - 1] + ln[hi - 1]) - first
            d_data.upload(data[first:first + size])
            d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
            batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, size, abi.DESC_PACKED, 0)
            select = None
            if filters:
                ctx.run_device(batch, abi.Outputs(None, 0, d_ver.ptr, None, None, None))
                select = d_ver
            ctx.flow_track_update(d_state, batch, d_scratch, need, d_res, select=select, flow_id=d_ids)
            ctx.flow_seq(batch, d_ids, select, d_seq_tab, cap, d_seq_scratch, seq_need, d_seq_res, max_packets=a.max_packets,
                         max_bytes=a.max_bytes, flags=abi.FLOW_SEQ_KEEP_UNKEYED, out_select=d_sel)
            ctx.pass_pack(batch, d_sel, d_pack, d_pack.nbytes, d_tot, d_np, lead=LEAD)
            ctx.synchronize()
            total, count = int(d_tot.download(np.zeros(1, np.uint64))[0]), int(d_np.download(np.zeros(2, np.uint32))[0])
            r = abi.FlowSeqResult.from_bytes(d_seq_res.download(np.zeros(64, np.uint8))).as_dict()
            if r["bad_ids"]:
                raise SystemExit("pcap_cutoff: the tracker's flow ids do not fit the sequence table")
            if total > d_pack.nbytes or count != r["kept"]:
                raise SystemExit("pcap_cutoff: the pack disagrees with the selection")
            if total:
                fh.write(d_pack.download(np.zeros(total, np.uint8)).tobytes())   # only the packed bytes cross PCIe
            for k in ("selected", "numbered", "unkeyed"):
                out[k] += r[k]
            out["written_packets"] += count
            out["written_bytes"] += total - LEAD * count
        hdr = abi.FlowTrackHdr.from_bytes(d_state.download(np.zeros(128, np.uint8))).as_dict()
        if hdr["overflow_packets"]:
            raise SystemExit(f"pcap_cutoff: more than --flow-cap {cap} flows: their packets could not be numbered, the output is removed")
        out["flows"] = hdr["n_flows"]
        abi.Context.flow_track_forget(d_state)   # before its memory goes back
        for b in bufs:
            b.free()
        whole = True
    except abi.BtError as e:
        raise SystemExit(f"pcap_cutoff: {e}")
    finally:
        if fh is not None:
            fh.close()
            if not whole:   # an error or an overflow: no partial output stays behind
                os.remove(a.dst)
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

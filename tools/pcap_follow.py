#!/usr/bin/env python3
"""Follow every TCP stream of a pcap file on the GPU: one file of reassembled payload bytes per (flow,
direction), as `tcpflow` and Wireshark's "follow TCP stream" produce.

    tools/pcap_follow.py --in a.pcap --out-dir DIR [--filter TYPE:EXPR[:PRIO]]... [--bidirectional]
                         [--flow-cap N] [--chunk PACKETS] [--device D]

Per chunk of the file: the filter (if any), the flow tracker's update (bt_flow_track_update_device, which
numbers the flows), bt_flow_tcpseq_device (every segment's place in its direction's sequence space) and
bt_flow_follow_device without a pattern (the segments in sequence order, overlaps trimmed, the delivered bytes
written out), the last two with the filter's verdict as `select`. Only the runs and the delivered bytes come
back from the device; each run is appended to DIR/<src>.<sport>-<dst>.<dport>, named from the tracker's flow
record as tcpflow names its files (IPv4 addresses and ports zero-padded). The reorder window is the chunk: a
segment that fills a hole of an earlier chunk is late and dropped. A run behind a hole is appended as it is:
holes are reported, not filled.

Prints one line per stream in order of (flow, direction): its file name, bytes, runs and holes; and a JSON line
of totals on stderr.
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


def stream_name(rec, direction: int) -> str:
    """tcpflow's file name of one direction of a tracker record: the record's key is the forward direction's."""
    klass, key = int(rec["klass"]), rec["key"].tobytes()
    alen = 4 if klass in (abi.FLOW_V4, abi.FLOW_V4_L4) else 16
    ends = [[ipaddress.ip_address(key[:alen]), int.from_bytes(key[2 * alen:2 * alen + 2], "big")],
            [ipaddress.ip_address(key[alen:2 * alen]), int.from_bytes(key[2 * alen + 2:2 * alen + 4], "big")]]
    if direction:
        ends.reverse()
    show = lambda e: (".".join(f"{b:03d}" for b in e[0].packed) if alen == 4 else str(e[0]).replace(":", "_")) + f".{e[1]:05d}"  # noqa: E731
    return f"{show(ends[0])}-{show(ends[1])}"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True)
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--bidirectional", action="store_true")
    ap.add_argument("--flow-cap", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0, metavar="PACKETS")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.chunk < 0 or a.flow_cap < 0:
        raise SystemExit("--chunk / --flow-cap: want a positive count")
    filters = [parse_filter(f) for f in a.filter]
    data = np.fromfile(a.src, np.uint8)
    try:
        info, desc = abi.pcap_index(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_follow: {e}")
    os.makedirs(a.out_dir, exist_ok=True)
    flags = abi.FLOWTAB_BIDIRECTIONAL if a.bidirectional else 0
    off, ln = (desc & MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    parts = list(chunks_of(off, ln, a.chunk))
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) for lo, hi in parts), default=1)
    cap = a.flow_cap or max(1, len(off))
    streams: dict = {}   # (flow, direction) -> [bytes, runs, holes]
    names: dict = {}
    totals = {"packets": int(len(desc)), "chunks": len(parts), "stream_bytes": 0, "runs": 0, "holes": 0, "late_packets": 0, "dup_packets": 0}
    ctx = abi.Context(a.device)
    try:
        if any(s.kind == K_HOST for s in ctx.compile(filters)):
            raise SystemExit("pcap_follow: a filter the GPU cannot decide (a CUSTOM callback, a PAYLOAD regex outside its subset) is in the program")
        lay = abi.flow_track_layout(cap)
        need, qneed, fneed = abi.flow_track_scratch_bytes(max_n), abi.flow_tcpseq_scratch_bytes(max_n, cap), abi.flow_follow_scratch_bytes(max_n, cap)
        out_cap = (max_bytes + 255) // 256 * 256
        d_state, d_scratch, d_res = ctx.alloc(lay["total"]), ctx.alloc(need), ctx.alloc(64)
        d_data, d_desc = ctx.alloc(out_cap + 256), ctx.alloc(max(16, max_n * 8))
        d_ver, d_ids, d_off = ctx.alloc(max(16, (max_n + 63) // 64 * 8)), ctx.alloc(max(16, max_n * 4)), ctx.alloc(max(16, max_n * 8))
        d_seq, d_qscratch, d_qres = ctx.alloc(128 * cap), ctx.alloc(max(256, qneed)), ctx.alloc(64)
        d_tab, d_fscratch, d_rres, d_fres = ctx.alloc(128 * cap), ctx.alloc(max(256, fneed)), ctx.alloc(64), ctx.alloc(32)
        d_out, d_runs = ctx.alloc(out_cap), ctx.alloc(max(32, 32 * max_n))
        bufs = [d_state, d_scratch, d_res, d_data, d_desc, d_ver, d_ids, d_off, d_seq, d_qscratch, d_qres, d_tab, d_fscratch, d_rres, d_fres, d_out, d_runs]
        d_seq.zero()
        d_tab.zero()
        ctx.reserve(max_n)
        ctx.flow_track_init(d_state, lay["total"], cap, flags)
        recs = np.zeros(0, abi.FlowTrackRec)
        for lo, hi in parts:
            n, first = hi - lo, int(off[lo])
            nbytes = int(off[hi - 1] + ln[hi - 1]) - first
            d_data.upload(data[first:first + nbytes])
            d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
            batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, max(nbytes, 1), abi.DESC_PACKED, 0)
            sel = d_ver if filters else None
            if filters:
                ctx.run_device(batch, abi.Outputs(None, 0, d_ver.ptr, None, None, None))
            ctx.flow_track_update(d_state, batch, d_scratch, need, d_res, select=sel, flow_id=d_ids)
            ctx.flow_tcpseq(batch, d_ids, sel, flags, d_seq, cap, d_qscratch, qneed, d_qres, off=d_off)
            ctx.flow_follow(batch, d_ids, sel, d_off, flags, None, None, d_tab, cap, d_fscratch, fneed, d_rres, d_fres,
                            out_bytes=d_out, cap=out_cap, runs=d_runs, run_cap=n)
            ctx.synchronize()
            hdr = abi.FlowTrackHdr.from_bytes(d_state.download(np.zeros(128, np.uint8))).as_dict()
            if hdr["overflow_packets"]:
                raise SystemExit(f"pcap_follow: more than --flow-cap {cap} flows at once")
            res = abi.FlowReasmResult.from_bytes(d_rres.download(np.zeros(64, np.uint8))).as_dict()
            fres = abi.FlowFollowResult.from_bytes(d_fres.download(np.zeros(32, np.uint8))).as_dict()
            assert fres["written"] == fres["total"] and fres["runs_written"] == fres["n_runs"]   # cap >= the chunk's bytes, run_cap = n
            totals["stream_bytes"] += fres["total"]
            totals["runs"] += fres["n_runs"]
            totals["late_packets"] += res["late_packets"]
            totals["dup_packets"] += res["dup_packets"]
            if not fres["n_runs"]:
                continue
            if hdr["n_flows"] > len(recs):   # the records of the flows this chunk met first: only they come back
                both = d_state.download(np.zeros(lay["records"] + 104 * hdr["n_flows"], np.uint8))
                recs = both[lay["records"]:].view(abi.FlowTrackRec)
            runs = d_runs.download(np.zeros(32 * fres["n_runs"], np.uint8)).view(abi.FlowFollowRun)
            got = d_out.download(np.zeros(fres["written"], np.uint8))
            for u in runs:   # ascending (flow, direction): a stream's runs of the chunk are neighbours
                key = (int(u["flow"]), int(u["flags"]) & abi.FOLLOW_DIR)
                if key not in names:
                    names[key] = stream_name(recs[key[0]], key[1])
                    open(os.path.join(a.out_dir, names[key]), "wb").close()
                    streams[key] = [0, 0, 0]
                with open(os.path.join(a.out_dir, names[key]), "ab") as fh:
                    fh.write(got[int(u["at"]):int(u["at"] + u["len"])].tobytes())
                s = streams[key]
                s[0] += int(u["len"])
                s[1] += 1
                s[2] += bool(int(u["flags"]) & abi.FOLLOW_HOLE)
        abi.Context.flow_track_forget(d_state)   # before its memory goes back
        for b in bufs:
            b.free()
    except abi.BtError as e:
        raise SystemExit(f"pcap_follow: {e}")
    finally:
        ctx.close()
    for key in sorted(streams):
        b, r, h = streams[key]
        print(f"{names[key]} bytes={b} runs={r} holes={h}")
        totals["holes"] += h
    totals["streams"] = len(streams)
    print(json.dumps(totals), file=sys.stderr)


if __name__ == "__main__":
    main()

"""List the flows of a classic pcap capture from the GPU's flow table: one line per flow with its
class, addresses, ports, packets and bytes per direction, and the first and last packet number in
the file (the NetFlow / conntrack view of a capture).

Usage: python tools/pcap_flows.py --in a.pcap [--filter TYPE:EXPR[:PRIO] ...] [--bidirectional] [--l3-only]
                                  [--top N] [--format csv|json] [--chunk-packets N]
                                  [--track [--idle SECONDS] [--flow-cap N] [--tcp [--closed-idle SECONDS]]
                                           [--stats] [--seq] [--reasm EXPR] [--by bytes|packets|duration|syn|rst]
                                           [--hosts [--top N --by bytes|packets|flows]]]
  --filter         as tools/pcap_filter.py takes it; only passing packets are counted
  --bidirectional  both directions of a conversation are one flow (BT_FLOWTAB_BIDIRECTIONAL): the
                   listed source is the smaller endpoint, packets_rev / bytes_rev count the other direction
  --l3-only        never key on ports (BT_FLOWTAB_L3_ONLY)
  --top N          the N flows with the most bytes, largest first (default: every flow, by first packet)
  --format         csv (default, with a header line) or json (one object per line)
  --chunk-packets  packets per device batch (default: at most 64 MiB of the file and 1M packets)
  --track          keep one flow tracker on the device for the whole file (bt_flow_track_update_device): no
                   download and no merge per chunk, one wait and one read of its header and records at the
                   end. The output is that of the default path, byte for byte.
  --idle SECONDS   with --track: after each chunk, the flows whose last packet is more than SECONDS older than
                   the chunk's last packet (by the pcap record headers' timestamps) age out
                   (bt_flow_track_expire_device) and are printed at once, the others at the end; a flow that comes
                   back is a new line. Adds the columns first_ts and last_ts (seconds, with the file's six or nine decimals).
  --flow-cap N     with --track: room for N flows (default: one per packet of the file)
  --tcp            with --track: a TCP side table beside the tracker (bt_flow_tcp_update_device behind every update).
                   Adds the columns tcp_flags_fwd and tcp_flags_rev (the union of the TCP flags byte per direction,
                   hexadecimal), tcp_state (bt_flow_tcp_state: none, opening, established, closing, closed, reset,
                   midstream; a function of the two unions, not a sequence-checked machine), syn, fin and rst
                   (packets with SYN and no ACK, with FIN, with RST). Still one wait without --idle.
  --closed-idle SECONDS  with --tcp and --idle: a closed or reset connection ages out once its last packet is more
                   than SECONDS older than the chunk's last packet (bt_flow_track_expire_tcp_device)
  --stats          with --track (with or without --tcp): a statistics side table beside the tracker
                   (bt_flow_stat_update_device behind every update). Adds the columns protocols (tcp, udp, icmp, icmp6,
                   other: every kind seen on the flow, joined by +), proto_max, and per direction (the second with the
                   suffix _rev) len_min, len_mean, len_max, len_stddev (frame lengths; the mean and the population
                   standard deviation from the flow record's packets and bytes and the sum of squares, three decimals),
                   ttl_min, ttl_max, payload_bytes and payload_packets (L4 payload by the IP and TCP header fields); with
                   --bidirectional also initiator (fwd or rev: who sent the first SYN), rtt_server (SYN to SYN-ACK) and
                   rtt_client (SYN-ACK to ACK) in the capture's time unit (micro- or nanoseconds), empty where the
                   handshake was not seen. With --idle the statistics of a flow that ages out leave with it
                   (bt_flow_track_side_move_device behind the expire). Not with --top or --hosts.
  --seq            with --track: a TCP sequence side table beside the tracker (bt_flow_tcpseq_device behind every
                   update). Adds per direction (the second with the suffix _rev) seq_packets (segments that take
                   sequence space), old_packets (retransmitted or late: every byte at or below the highest seen; with
                   gap_packets 0 certain duplicates), gap_packets (ahead of everything seen: a loss or reordering in
                   front), overlap_packets, old_bytes and gap_bytes. With --idle the record of a flow that ages out
                   leaves with it. Not with --top or --hosts.
  --reasm EXPR     with --track: a TCP reassembly side table beside the tracker (bt_flow_tcpseq_device, then
                   bt_flow_reasm_device behind every update): EXPR (a bounded-memory pattern, as tools/pcap_sessions.py
                   --stream takes it) is matched over each direction's bytes in sequence order, the segments of a chunk
                   reordered, overlaps trimmed, no match across a hole; a hole still open at a chunk's end is given up.
                   Adds per direction (the second with the suffix _rev) reasm_packets (segments that delivered a byte),
                   reasm_hits (packets in which a match ends), holes, hole_bytes, dup_packets, dup_bytes, late_packets,
                   late_bytes and delivered_to (the position up to which the stream was delivered, counted from the
                   direction's first-arrived segment; empty for a direction without data). With --idle the record of a
                   flow that ages out leaves with it. Not with --top or --hosts.
  --by MEASURE     with --track and --top N, N <= 4096: what the top is ordered by, largest first and the
                   earliest-seen flow first among equals: bytes (default), packets (both directions), duration
                   (last minus first packet time by the pcap record headers), syn or rst (with --tcp: packets with
                   SYN and no ACK, with RST)
  --hosts          with --track: the endpoint view instead of the flow list (bt_flow_track_hosts_device, one query
                   behind the last update): one line per address with the flows it is the first / second
                   endpoint of, packets and bytes sent and received, first and last seen (seconds by the pcap
                   record headers) and, with --tcp, its flows by connection state, the flows with SYN in the
                   direction it sends / receives, and SYN / FIN / RST packets. Hosts come in order of first
                   appearance; --top N keeps the N largest by --by bytes (sent + received, default), packets or
                   flows, sorted here from the host records read back. Not with --idle.
With --track and --top N, N <= 4096, the top is selected on the device (bt_flow_track_top_device behind the
last update): still one wait, then only the N records (and N side records with --tcp) are read. A larger N
downloads every record and sorts here, as the default path does.
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
TCP_COLUMNS = ("tcp_flags_fwd", "tcp_flags_rev", "tcp_state", "syn", "fin", "rst")
STAT_DIR_COLUMNS = ("len_min", "len_mean", "len_max", "len_stddev", "ttl_min", "ttl_max", "payload_bytes", "payload_packets")
STAT_COLUMNS = ("protocols", "proto_max") + STAT_DIR_COLUMNS + tuple(c + "_rev" for c in STAT_DIR_COLUMNS)
RTT_COLUMNS = ("initiator", "rtt_server", "rtt_client")
SEQ_DIR_COLUMNS = ("seq_packets", "old_packets", "gap_packets", "overlap_packets", "old_bytes", "gap_bytes")
SEQ_COLUMNS = SEQ_DIR_COLUMNS + tuple(c + "_rev" for c in SEQ_DIR_COLUMNS)
REASM_DIR_COLUMNS = ("reasm_packets", "reasm_hits", "holes", "hole_bytes", "dup_packets", "dup_bytes", "late_packets", "late_bytes",
                     "delivered_to")
REASM_COLUMNS = REASM_DIR_COLUMNS + tuple(c + "_rev" for c in REASM_DIR_COLUMNS)
U64_MAX = (1 << 64) - 1
HOST_COLUMNS = ("address", "flows_src", "flows_dst", "packets_sent", "bytes_sent", "packets_received", "bytes_received",
                "first_seen", "last_seen")
HOST_TCP_COLUMNS = tuple("tcp_" + n for n in abi.TCP_STATE_NAMES) + ("syn_flows_sent", "syn_flows_received", "syn", "fin", "rst")
HOSTS_BY = {"bytes": lambda r: r["bytes_sent"] + r["bytes_received"], "packets": lambda r: r["packets_sent"] + r["packets_received"],
            "flows": lambda r: r["flows_src"] + r["flows_dst"]}
TOP_BY = {"bytes": abi.FLOW_TOP_BYTES, "packets": abi.FLOW_TOP_PACKETS, "duration": abi.FLOW_TOP_DURATION,
          "syn": abi.FLOW_TOP_TCP_SYN, "rst": abi.FLOW_TOP_TCP_RST}


def describe(klass: int, key: bytes, v: list) -> dict:
    """One output line: v = [packets, packets_rev, bytes, bytes_rev, first, last]."""
    alen = 4 if klass in (abi.FLOW_V4, abi.FLOW_V4_L4) else 16
    ports = klass in (abi.FLOW_V4_L4, abi.FLOW_V6_L4)
    p = key[2 * alen:2 * alen + 4]
    return {"class": abi.FLOW_NAMES[klass], "src": str(ipaddress.ip_address(key[:alen])),
            "dst": str(ipaddress.ip_address(key[alen:2 * alen])),
            "sport": int.from_bytes(p[0:2], "big") if ports else None, "dport": int.from_bytes(p[2:4], "big") if ports else None,
            "packets": v[0], "bytes": v[2], "packets_rev": v[1], "bytes_rev": v[3], "first": v[4], "last": v[5]}


def describe_host(h, with_tcp: bool, unit: int, digits: int) -> dict:
    """One --hosts output line from a bt_flow_host_rec."""
    stamp = lambda v: f"{int(v) // unit}.{int(v) % unit:0{digits}d}"   # noqa: E731  exact: seconds, then the file's fraction
    r = {"address": str(ipaddress.ip_address(h["addr"].tobytes()[:4 if int(h["family"]) == 4 else 16])),
         "flows_src": int(h["flows"][0]), "flows_dst": int(h["flows"][1]),
         "packets_sent": int(h["packets"][0]), "bytes_sent": int(h["bytes"][0]),
         "packets_received": int(h["packets"][1]), "bytes_received": int(h["bytes"][1]),
         "first_seen": stamp(h["first_ts"]), "last_seen": stamp(h["last_ts"])}
    if with_tcp:
        for k, name in enumerate(abi.TCP_STATE_NAMES):
            r["tcp_" + name] = int(h["tcp_state"][k])
        r["syn_flows_sent"], r["syn_flows_received"] = int(h["syn_flows"][0]), int(h["syn_flows"][1])
        r["syn"], r["fin"], r["rst"] = int(h["syn_packets"]), int(h["fin_packets"]), int(h["rst_packets"])
    return r


def describe_stats(r: dict, rec, packets, nbytes, bidirectional: bool):
    """The --stats columns of one output line from a bt_flow_stat_rec and the flow record's packets and bytes per direction."""
    d = abi.decode_flow_stat(rec)
    r["protocols"], r["proto_max"] = "+".join(d["protocols"]), d["proto_max"]
    for k, suffix in enumerate(("", "_rev")):
        n, b, sq = packets[k], nbytes[k], d["len_sq"][k]
        seen = d["len_min"][k] is not None
        r["len_min" + suffix], r["len_max" + suffix] = d["len_min"][k], d["len_max"][k]
        r["len_mean" + suffix] = f"{b / n:.3f}" if seen and n else None
        r["len_stddev" + suffix] = f"{max(0, n * sq - b * b) ** 0.5 / n:.3f}" if seen and n else None   # exact up to the root
        r["ttl_min" + suffix], r["ttl_max" + suffix] = d["ttl_min"][k], d["ttl_max"][k]
        r["payload_bytes" + suffix], r["payload_packets" + suffix] = d["payload_bytes"][k], d["payload_packets"][k]
    if bidirectional:
        t = abi.flow_stat_rtt(rec)
        r["initiator"] = ("fwd", "rev")[t["initiator"]] if t["has_initiator"] else None
        r["rtt_server"] = t["rtt_server"] if t["server_valid"] else None
        r["rtt_client"] = t["rtt_client"] if t["client_valid"] else None


def describe_seq(r: dict, rec):
    """The --seq columns of one output line from a bt_flow_tcpseq_rec."""
    d = abi.decode_flow_tcpseq(rec)
    for k, suffix in enumerate(("", "_rev")):
        for c in SEQ_DIR_COLUMNS:
            r[c + suffix] = d[c][k]


def describe_reasm(r: dict, rec):
    """The --reasm columns of one output line from a bt_flow_reasm_rec."""
    d = abi.decode_flow_reasm(rec)
    names = {"reasm_packets": "stream_packets", "reasm_hits": "hit_packets"}
    for k, suffix in enumerate(("", "_rev")):
        for c in REASM_DIR_COLUMNS[:-1]:
            r[c + suffix] = d[names.get(c, c)][k]
        r["delivered_to" + suffix] = d["next"][k] if d["have"][k] else None


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


def track(a, ctx, filters, flags, data, info, off, ln, parts, totals) -> list:
    """The --track path: every chunk merged into one tracker on the device. Returns the output lines'
    dicts in output order and fills totals."""
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) for lo, hi in parts), default=1)
    cap = a.flow_cap or max(1, len(off))
    lay = abi.flow_track_layout(cap)
    need, xneed = abi.flow_track_scratch_bytes(max_n), abi.flow_track_expire_scratch_bytes(cap)
    unit = 1_000_000_000 if info["nanosecond"] else 1_000_000
    starts = np.array([lo for lo, _ in parts] + [0], np.int64)
    timed = a.idle is not None
    on_device = 0 < a.top <= abi.FLOW_TOP_MAX_K and not a.hosts   # the top comes from the device (--idle with --top is refused)
    stamped = timed or (on_device and a.by == "duration") or a.hosts or a.stats
    if stamped:   # a record's header is the 16 bytes before its data: ts_sec, ts_frac in the file's byte order
        head = np.stack([data[off - 16 + k] for k in range(8)], axis=1).astype(np.uint64) if len(off) else np.zeros((0, 8), np.uint64)
        order = (3, 2, 1, 0) if info["swapped"] else (0, 1, 2, 3)
        word = lambda b: sum(head[:, b + order[k]] << np.uint64(8 * k) for k in range(4))  # noqa: E731
        ts = word(0) * np.uint64(unit) + word(4)
    rows = []

    def lines(recs, side=None, stat=None, seq=None, reasm=None):
        for k, f in enumerate(recs):
            v = [int(f["packets"][0]), int(f["packets"][1]), int(f["bytes"][0]), int(f["bytes"][1]),
                 int(starts[f["first_batch"]]) + int(f["first"]), int(starts[f["last_batch"]]) + int(f["last"])]
            r = describe(int(f["klass"]), f["key"].tobytes(), v)
            if timed:
                digits = 9 if info["nanosecond"] else 6   # exact: seconds, then the file's fraction
                r["first_ts"], r["last_ts"] = (f"{int(f[c]) // unit}.{int(f[c]) % unit:0{digits}d}" for c in ("first_ts", "last_ts"))
            if side is not None:
                t = side[k]
                fwd, rev = int(t["flags"][0]), int(t["flags"][1])
                r["tcp_flags_fwd"], r["tcp_flags_rev"] = f"0x{fwd:02x}", f"0x{rev:02x}"
                r["tcp_state"] = abi.TCP_STATE_NAMES[abi.flow_tcp_state(fwd, rev, flags)]
                r["syn"], r["fin"], r["rst"] = int(t["syn_packets"]), int(t["fin_packets"]), int(t["rst_packets"])
            if stat is not None:
                describe_stats(r, stat[k], v[0:2], v[2:4], bool(flags & abi.FLOWTAB_BIDIRECTIONAL))
            if seq is not None:
                describe_seq(r, seq[k])
            if reasm is not None:
                describe_reasm(r, reasm[k])
            rows.append(r)

    if a.tcp and timed:
        xneed = abi.flow_track_expire_tcp_scratch_bytes(cap)
    d_state, d_scratch, d_res = ctx.alloc(lay["total"]), ctx.alloc(need), ctx.alloc(64)
    d_data = ctx.alloc((max_bytes + 255) // 256 * 256 + 256)
    d_desc, d_ver = ctx.alloc(max(16, max_n * 8)), ctx.alloc(max(16, (max_n + 63) // 64 * 8))
    bufs = [d_state, d_scratch, d_res, d_data, d_desc, d_ver]
    if timed:
        d_ts, d_xscratch, d_xres, d_exp = ctx.alloc(max(16, max_n * 8)), ctx.alloc(xneed), ctx.alloc(32), ctx.alloc(104 * cap)
        bufs += [d_ts, d_xscratch, d_xres, d_exp]
    seqd = a.seq or a.reasm is not None   # the reassembly takes its offsets from the sequence spaces
    sided = a.stats or seqd   # side tables that follow an expire's remap
    if a.tcp or sided:   # the update's flow ids feed the side tables
        d_ids = ctx.alloc(max(16, max_n * 4))
        bufs.append(d_ids)
    if sided and timed:
        mneed = abi.flow_track_side_move_scratch_bytes(cap, 128)
        d_remap, d_mscratch = ctx.alloc(4 * cap), ctx.alloc(mneed)
        bufs += [d_remap, d_mscratch]
    if a.stats:   # the statistics, zeroed once; with --idle they follow the expire's remap
        d_stat, d_sres = ctx.alloc(128 * cap), ctx.alloc(32)
        d_stat.zero()
        bufs += [d_stat, d_sres]
        if timed:
            d_exp_stat = ctx.alloc(128 * cap)
            bufs.append(d_exp_stat)
    if seqd:   # the sequence spaces, zeroed once; with --idle they follow the expire's remap
        qneed = abi.flow_tcpseq_scratch_bytes(max_n, cap)
        d_seq, d_qscratch, d_qres = ctx.alloc(128 * cap), ctx.alloc(max(256, qneed)), ctx.alloc(64)
        d_seq.zero()
        bufs += [d_seq, d_qscratch, d_qres]
        if timed:
            d_exp_seq = ctx.alloc(128 * cap)
            bufs.append(d_exp_seq)
    if a.reasm is not None:   # the reassembly records, zeroed once; with --idle they follow the expire's remap
        rneed = abi.flow_reasm_scratch_bytes(max_n, cap)
        d_reasm, d_rscratch, d_rres = ctx.alloc(128 * cap), ctx.alloc(max(256, rneed)), ctx.alloc(64)
        d_off, d_blob = ctx.alloc(max(16, 8 * max_n)), ctx.alloc(len(a.blob))
        d_reasm.zero()
        d_blob.upload(a.blob)
        bufs += [d_reasm, d_rscratch, d_rres, d_off, d_blob]
        if timed:
            d_exp_reasm = ctx.alloc(128 * cap)
            bufs.append(d_exp_reasm)
    if a.tcp:   # the side table, zeroed once
        d_tcp, d_tres = ctx.alloc(16 * cap), ctx.alloc(32)
        d_tcp.zero()
        bufs += [d_tcp, d_tres]
        if timed:
            d_exp_tcp = ctx.alloc(16 * cap)
            bufs.append(d_exp_tcp)
        closed = U64_MAX if a.closed_idle is None else int(a.closed_idle * unit)
    if stamped and not timed:
        d_ts = ctx.alloc(max(16, max_n * 8))
        bufs.append(d_ts)
    if on_device:
        tneed = abi.flow_track_top_scratch_bytes(cap, a.top)
        d_tscratch, d_top, d_top_tcp, d_top_res = ctx.alloc(tneed), ctx.alloc(104 * a.top), ctx.alloc(16 * a.top), ctx.alloc(48)
        bufs += [d_tscratch, d_top, d_top_tcp, d_top_res]
    if a.hosts:   # room for every host: two per flow
        hneed = abi.flow_track_hosts_scratch_bytes(cap)
        d_hscratch, d_hosts, d_hres = ctx.alloc(hneed), ctx.alloc(128 * 2 * cap), ctx.alloc(64)
        bufs += [d_hscratch, d_hosts, d_hres]
    ctx.reserve(max_n)
    ctx.flow_track_init(d_state, lay["total"], cap, flags)
    for lo, hi in parts:
        n, first = hi - lo, int(off[lo])
        nbytes = int(off[hi - 1] + ln[hi - 1]) - first
        d_data.upload(data[first:first + nbytes])   # waits for the context's stream: the last chunk is done
        d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
        if stamped:
            d_ts.upload(ts[lo:hi])
        batch = abi.Batch(d_data.ptr, d_desc.ptr, 0, n, max(nbytes, 1), abi.DESC_PACKED, 0)
        if filters:
            ctx.run_device(batch, abi.Outputs(None, 0, d_ver.ptr, None, None, None))
        ctx.flow_track_update(d_state, batch, d_scratch, need, d_res, select=d_ver if filters else None,
                              ts=d_ts if stamped else None, flow_id=d_ids if a.tcp or sided else None)
        if a.tcp:
            ctx.flow_tcp_update(batch, d_ids, flags, d_tcp, cap, d_tres)
        if a.stats:
            ctx.flow_stat_update(batch, d_ids, flags, d_stat, cap, d_sres, ts=d_ts)
        if seqd:   # unselected packets carry the UNSELECTED sentinel: they are in no sequence space
            ctx.flow_tcpseq(batch, d_ids, None, flags, d_seq, cap, d_qscratch, qneed, d_qres, off=d_off if a.reasm is not None else None)
        if a.reasm is not None:   # the chunk's segments in sequence order, behind their offsets
            ctx.flow_reasm(batch, d_ids, None, d_off, flags, a.blob, d_blob, d_reasm, cap, d_rscratch, rneed, d_rres)
        if timed:   # what aged out is printed now: its count and records come back, nothing else
            if a.tcp:
                ctx.flow_track_expire_tcp(d_state, int(ts[hi - 1]), int(a.idle * unit), closed, d_tcp, d_xscratch, xneed, d_xres,
                                          expired=d_exp, expired_cap=cap, expired_tcp=d_exp_tcp, remap=d_remap if sided else None)
            else:
                ctx.flow_track_expire(d_state, int(ts[hi - 1]), int(a.idle * unit), d_xscratch, xneed, d_xres, expired=d_exp, expired_cap=cap,
                                      remap=d_remap if sided else None)
            if a.stats:   # the statistics of the flows that stay move up, those of the flows that leave come out
                ctx.flow_track_side_move(d_stat, 128, cap, d_remap, d_xres, d_mscratch, mneed, expired_side=d_exp_stat, expired_cap=cap)
            if seqd:   # and so do the sequence spaces
                ctx.flow_track_side_move(d_seq, 128, cap, d_remap, d_xres, d_mscratch, mneed, expired_side=d_exp_seq, expired_cap=cap)
            if a.reasm is not None:   # and the reassembly records
                ctx.flow_track_side_move(d_reasm, 128, cap, d_remap, d_xres, d_mscratch, mneed, expired_side=d_exp_reasm, expired_cap=cap)
            ctx.synchronize()
            x = abi.FlowTrackExpireResult.from_bytes(d_xres.download(np.zeros(32, np.uint8))).as_dict()
            if x["n_expired"]:
                lines(d_exp.download(np.zeros(104 * x["n_expired"], np.uint8)).view(abi.FlowTrackRec),
                      d_exp_tcp.download(np.zeros(16 * x["n_expired"], np.uint8)).view(abi.FlowTcpRec) if a.tcp else None,
                      d_exp_stat.download(np.zeros(128 * x["n_expired"], np.uint8)).view(abi.FlowStatRec) if a.stats else None,
                      d_exp_seq.download(np.zeros(128 * x["n_expired"], np.uint8)).view(abi.FlowTcpseqRec) if a.seq else None,
                      d_exp_reasm.download(np.zeros(128 * x["n_expired"], np.uint8)).view(abi.FlowReasmRec) if a.reasm is not None else None)
    if on_device:   # behind the last update and side table update, on their stream
        ctx.flow_track_top(d_state, TOP_BY[a.by], a.top, d_tscratch, tneed, d_top_res, top=d_top, tcp=d_tcp if a.tcp else None,
                           top_tcp=d_top_tcp if a.tcp else None)
    if a.hosts:   # one query at the end of the capture, behind the last update and side table update
        ctx.flow_track_hosts(d_state, 2 * cap, d_hscratch, hneed, d_hres, hosts=d_hosts, tcp=d_tcp if a.tcp else None)
    ctx.synchronize()   # the one wait of the plain --track path
    hdr = abi.FlowTrackHdr.from_bytes(d_state.download(np.zeros(128, np.uint8))).as_dict()
    if hdr["overflow_packets"]:
        raise SystemExit(f"pcap_flows: more than --flow-cap {cap} flows at once")
    if a.hosts:
        totals["flows"] = hdr["n_flows"]
        res = abi.FlowHostsResult.from_bytes(d_hres.download(np.zeros(64, np.uint8))).as_dict()
        if res["status"] or res["overflow_endpoints"] or res["n_flows"] != hdr["n_flows"]:   # 4 flow_cap slots hold any 2 n_flows hosts
            raise SystemExit("pcap_flows: the endpoint query did not see the tracker")
        totals["hosts"], totals["hosts_v4"], totals["hosts_v6"] = res["n_hosts"], res["hosts_v4"], res["hosts_v6"]
        if res["n_written"]:   # only the host records cross PCIe
            digits = 9 if info["nanosecond"] else 6
            rows += [describe_host(h, a.tcp, unit, digits)
                     for h in d_hosts.download(np.zeros(128 * res["n_written"], np.uint8)).view(abi.FlowHostRec)]
    elif on_device:
        totals["flows"] = hdr["n_flows"]   # not the lines printed
        res = abi.FlowTopResult.from_bytes(d_top_res.download(np.zeros(48, np.uint8))).as_dict()
        if res["status"] or res["n_flows"] != hdr["n_flows"]:
            raise SystemExit("pcap_flows: the top-K query did not see the tracker")
        if res["n_top"]:   # only the top's records cross PCIe
            lines(d_top.download(np.zeros(104 * res["n_top"], np.uint8)).view(abi.FlowTrackRec),
                  d_top_tcp.download(np.zeros(16 * res["n_top"], np.uint8)).view(abi.FlowTcpRec) if a.tcp else None)
    elif hdr["n_flows"]:
        both = d_state.download(np.zeros(lay["records"] + 104 * hdr["n_flows"], np.uint8))
        lines(both[lay["records"]:].view(abi.FlowTrackRec),
              d_tcp.download(np.zeros(16 * hdr["n_flows"], np.uint8)).view(abi.FlowTcpRec) if a.tcp else None,
              d_stat.download(np.zeros(128 * hdr["n_flows"], np.uint8)).view(abi.FlowStatRec) if a.stats else None,
              d_seq.download(np.zeros(128 * hdr["n_flows"], np.uint8)).view(abi.FlowTcpseqRec) if a.seq else None,
              d_reasm.download(np.zeros(128 * hdr["n_flows"], np.uint8)).view(abi.FlowReasmRec) if a.reasm is not None else None)
    totals["selected"], totals["no_key"] = hdr["selected_packets"], hdr["none_packets"]
    abi.Context.flow_track_forget(d_state)   # before its memory goes back
    for b in bufs:
        b.free()
    return rows


def per_chunk(ctx, filters, flags, data, off, ln, parts, max_n, max_bytes, table, totals):
    """The default path: a per-batch table, a download of its records and a merge by key per chunk."""
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
    ap.add_argument("--track", action="store_true")
    ap.add_argument("--idle", type=float, default=None, metavar="SECONDS")
    ap.add_argument("--flow-cap", type=int, default=0)
    ap.add_argument("--tcp", action="store_true")
    ap.add_argument("--closed-idle", type=float, default=None, metavar="SECONDS")
    ap.add_argument("--by", choices=tuple(TOP_BY) + ("flows",), default=None)
    ap.add_argument("--hosts", action="store_true")
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--seq", action="store_true")
    ap.add_argument("--reasm", default=None, metavar="EXPR")
    a = ap.parse_args()
    if a.chunk_packets < 0 or a.top < 0:
        raise SystemExit("--chunk-packets / --top: want a positive count")
    if (a.idle is not None or a.flow_cap) and not a.track:
        raise SystemExit("--idle / --flow-cap: only with --track")
    if a.idle is not None and (a.idle < 0 or a.top):
        raise SystemExit("--idle: want a time in seconds >= 0, and no --top (flows are printed as they age out)")
    if a.tcp and not a.track:
        raise SystemExit("--tcp: only with --track")
    if a.closed_idle is not None and (not a.tcp or a.idle is None or a.closed_idle < 0):
        raise SystemExit("--closed-idle: want a time in seconds >= 0, with --tcp and --idle")
    if a.flow_cap < 0:
        raise SystemExit("--flow-cap: want a positive count")
    if a.stats and (not a.track or a.top or a.hosts):
        raise SystemExit("--stats: only with --track, and without --top and --hosts")
    if a.seq and (not a.track or a.top or a.hosts):
        raise SystemExit("--seq: only with --track, and without --top and --hosts")
    if a.reasm is not None and (not a.track or a.top or a.hosts):
        raise SystemExit("--reasm: only with --track, and without --top and --hosts")
    if a.reasm is not None:
        try:
            a.blob, _ = abi.flow_stream_compile(a.reasm)
        except abi.BtError as e:
            raise SystemExit(f"pcap_flows: --reasm: {e}")
    if a.hosts and (not a.track or a.idle is not None):
        raise SystemExit("--hosts: only with --track, and without --idle")
    if a.hosts and a.by is not None and (a.by not in HOSTS_BY or not a.top):
        raise SystemExit("--hosts --by: bytes, packets or flows, with --top N")
    if not a.hosts and a.by == "flows":
        raise SystemExit("--by flows: only with --hosts")
    if not a.hosts and a.by is not None and not (a.track and 0 < a.top <= abi.FLOW_TOP_MAX_K):
        raise SystemExit(f"--by: only with --track and --top N, N <= {abi.FLOW_TOP_MAX_K}")
    if a.by in ("syn", "rst") and not a.tcp:
        raise SystemExit("--by syn / rst: only with --tcp")
    a.by = a.by or "bytes"
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
    tracked = None
    try:
        if any(s.kind == K_HOST for s in ctx.compile(filters)):
            raise SystemExit("pcap_flows: a filter the GPU cannot decide (a CUSTOM callback, a PAYLOAD regex outside "
                             "its subset) is in the program")
        if a.track:
            tracked = track(a, ctx, filters, flags, data, info, off, ln, parts, totals)
        else:
            per_chunk(ctx, filters, flags, data, off, ln, parts, max_n, max_bytes, table, totals)
    except abi.BtError as e:
        raise SystemExit(f"pcap_flows: {e}")
    finally:
        ctx.close()
    rows = [describe(k[0], k[1], v) for k, v in table.items()] if tracked is None else tracked   # insertion order: by first packet
    columns = COLUMNS + (("first_ts", "last_ts") if a.idle is not None else ()) + (TCP_COLUMNS if a.tcp else ())
    if a.stats:
        columns += STAT_COLUMNS + (RTT_COLUMNS if a.bidirectional else ())
    if a.seq:
        columns += SEQ_COLUMNS
    if a.reasm is not None:
        columns += REASM_COLUMNS
    if a.hosts:   # host records in order of first appearance; a top is sorted here (stable: ties stay in that order)
        columns = HOST_COLUMNS + (HOST_TCP_COLUMNS if a.tcp else ())
        if a.top:
            rows = sorted(rows, key=lambda r: -HOSTS_BY[a.by](r))[:a.top]
    elif a.top and not (a.track and a.top <= abi.FLOW_TOP_MAX_K):   # otherwise the device selected and ordered them
        rows = sorted(rows, key=lambda r: (-(r["bytes"] + r["bytes_rev"]), r["first"]))[:a.top]
    if a.format == "csv":
        print(",".join(columns))
        for r in rows:
            print(",".join("" if r[c] is None else str(r[c]) for c in columns))
    else:
        for r in rows:
            print(json.dumps(r))
    totals["flows"] = len(table) if tracked is None else totals.get("flows", len(tracked))
    print(json.dumps(totals), file=sys.stderr)


if __name__ == "__main__":
    main()

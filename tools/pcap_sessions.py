"""Write every packet of every connection in which some packet passed the filters (or, with
--invert, drop those connections whole): the session view of tools/pcap_filter.py, decided on the GPU.

Usage: python tools/pcap_sessions.py --in a.pcap --out b.pcap --filter TYPE:EXPR[:PRIO] ...
                                     [--stream EXPR [--skip-retransmits | --reassemble]] [--bidirectional] [--l3-only] [--invert]
                                     [--flow-cap N] [--chunk PACKETS]
  --filter         as tools/pcap_filter.py takes it
  --stream EXPR    also (or, without --filter, only) select the connections in whose payload stream EXPR matches,
                   wherever the match lies: across TCP segments and past a packet's first 100 bytes
                   (bt_flow_stream_device, per direction, in arrival order). EXPR must have bounded memory: no +, *,
                   {n,}, ^, $ or \\b; anything else ends the run with the construct's name, never a per-packet match
  --skip-retransmits  with --stream: classify the TCP segments first (bt_flow_tcpseq_device) and keep those whose bytes
                   all lie at or below the highest sequence number seen (retransmitted or late) out of the stream, so
                   that HE, LL, LL again, O reads HELLO and not HELLLLO
  --reassemble     with --stream: match TCP in sequence order. bt_flow_tcpseq_device places every segment,
                   bt_flow_reasm_device orders each chunk's segments by position, trims what overlaps and cuts the
                   matcher at a hole, so LO before HEL still reads HELLO and a late segment that fills a hole is used;
                   everything it does not place (UDP) goes through bt_flow_stream_device in arrival order. The reorder
                   window is the chunk. It supersedes --skip-retransmits: giving both is an error
  --bidirectional  both directions of a conversation are one session (BT_FLOWTAB_BIDIRECTIONAL)
  --l3-only        never key on ports (BT_FLOWTAB_L3_ONLY): a session is a pair of addresses
  --invert         write the complement: every packet that is in no session with a passing packet
  --flow-cap N     room for N flows in the tracker (default: one per packet of the file)
  --chunk PACKETS  packets per device batch (default: at most 64 MiB of the file and 1M packets)
The file is taken in chunks of whole records, as tools/pcap_stats.py takes it, twice.
Pass one, per chunk: the filter-only bt_parse_filter_device, bt_flow_track_update_device over all
packets (one tracker for the whole file, so a flow keeps its number from chunk to chunk; the
chunk's flow ids and verdict words stay on the device) and bt_flow_mark_update_device with the
chunk's verdict as the hits. Nothing is waited for until the last chunk is enqueued; then the
tracker's header is read, and more flows than --flow-cap end the run before the output file is
opened: no partial session is ever written.
Pass two, per chunk: bt_flow_mark_select_device with op OR over the chunk's verdict (a passing
packet without a flow key is a session of its own, so the output always contains the plain
filter's), then bt_pass_pack_device with lead 16, so that the record headers go along. With
--invert the op is ANDNOT over the complement of the chunk's verdict (the verdict words of the
file, n / 8 bytes, are complemented here between the passes): a packet is written when it did not
pass and its flow carries no mark, exactly the packets the default run leaves out. Only the
packed bytes come back. The output records are verbatim and in order behind the input's global
header, as bt_pcap_filter writes them. A program with a slot the GPU cannot decide (BT_K_HOST) is refused.
With --stream, pass one per chunk is: the filter (if any), the tracker update, bt_flow_stream_device over all packets
against one stream table for the whole file, bt_flow_mark_update_device with the stream's hits (and, with a filter, a
second one with the verdict), then pass two as above; without a filter the stream's hit words stand where the verdict's do.
Prints one JSON line: packets, hit_packets, flows, marked_flows, unkeyed_hits, written_packets, written_bytes, and with
--stream also stream_packets, stream_bytes, stream_hit_packets, and with --skip-retransmits seq_packets and old_packets;
with --reassemble seq_packets, old_packets, reasm_packets, reasm_bytes, reasm_hit_packets, holes, dup_packets, late_packets
and far_packets. hit_packets stays what it is without the option: the verdict's hit packets, or without a filter the
arrival-order matcher's; the reassembly's are reasm_hit_packets, and marked_flows counts a flow whichever call marked it first.
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
MARK = 0x1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True)
    ap.add_argument("--out", dest="dst", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--stream", default=None, metavar="EXPR")
    ap.add_argument("--skip-retransmits", action="store_true")
    ap.add_argument("--reassemble", action="store_true")
    ap.add_argument("--bidirectional", action="store_true")
    ap.add_argument("--l3-only", action="store_true")
    ap.add_argument("--invert", action="store_true")
    ap.add_argument("--flow-cap", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0, metavar="PACKETS")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if a.chunk < 0 or a.flow_cap < 0:
        raise SystemExit("--chunk / --flow-cap: want a positive count")
    if not a.filter and a.stream is None:
        raise SystemExit("--filter: want at least one (without a filter every packet passes: copy the file)")
    if a.skip_retransmits and a.stream is None:
        raise SystemExit("--skip-retransmits: goes with --stream")
    if a.reassemble and a.stream is None:
        raise SystemExit("--reassemble: goes with --stream")
    if a.reassemble and a.skip_retransmits:
        raise SystemExit("--reassemble: supersedes --skip-retransmits, give one of them")
    filters = [parse_filter(f) for f in a.filter]
    blob = None
    if a.stream is not None:
        try:
            blob, _ = abi.flow_stream_compile(a.stream)
        except abi.BtError as e:   # never a silent per-packet match instead
            raise SystemExit(f"pcap_sessions: --stream: {e}")
    data = np.fromfile(a.src, np.uint8)
    try:
        info, desc = abi.pcap_index(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_sessions: {e}")
    flags = (abi.FLOWTAB_BIDIRECTIONAL if a.bidirectional else 0) | (abi.FLOWTAB_L3_ONLY if a.l3_only else 0)
    off, ln = (desc & MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    parts = list(chunks_of(off, ln, a.chunk))
    total_n = len(off)
    max_n = max((hi - lo for lo, hi in parts), default=1)
    max_bytes = max((int(off[hi - 1] + ln[hi - 1] - off[lo]) + LEAD for lo, hi in parts), default=1)
    word0 = np.cumsum([0] + [(hi - lo + 63) // 64 for lo, hi in parts])   # where each chunk's verdict words start
    cap = a.flow_cap or max(1, total_n)
    out = {"packets": total_n, "hit_packets": 0, "flows": 0, "marked_flows": 0, "unkeyed_hits": 0, "written_packets": 0, "written_bytes": 0}
    ctx = abi.Context(a.device)
    fh, whole = None, False
    try:
        if filters and any(s.kind == K_HOST for s in ctx.compile(filters)):
            raise SystemExit("pcap_sessions: a filter the GPU cannot decide (a CUSTOM callback, a PAYLOAD regex outside "
                             "its subset) is in the program")
        lay = abi.flow_track_layout(cap)
        need = abi.flow_track_scratch_bytes(max_n)
        d_state, d_scratch, d_res = ctx.alloc(lay["total"]), ctx.alloc(need), ctx.alloc(64)
        d_marks = ctx.alloc(32 * cap)
        d_ids, d_ver = ctx.alloc(max(16, 4 * total_n)), ctx.alloc(max(16, 8 * int(word0[-1])))
        d_mres = ctx.alloc(max(32, 32 * len(parts)))   # one result per chunk: read once, behind the last
        d_data = ctx.alloc((max_bytes + 255) // 256 * 256 + 256)
        d_desc = ctx.alloc(max(16, max_n * 8))
        d_sel, d_sres = ctx.alloc(max(16, (max_n + 63) // 64 * 8)), ctx.alloc(32)
        d_pack, d_tot, d_np = ctx.alloc(max_bytes + LEAD * max_n + 256), ctx.alloc(8), ctx.alloc(8)
        bufs = [d_state, d_scratch, d_res, d_marks, d_ids, d_ver, d_mres, d_data, d_desc, d_sel, d_sres, d_pack, d_tot, d_np]
        if blob is not None:
            sneed = abi.flow_stream_scratch_bytes(max_n, cap)
            d_blob, d_stab, d_sscr = ctx.alloc(len(blob)), ctx.alloc(32 * cap), ctx.alloc(max(256, sneed))
            d_hit = ctx.alloc(max(16, (max_n + 63) // 64 * 8)) if filters else None   # beside the verdict, or in its place
            d_stres, d_mres2 = ctx.alloc(max(64, 64 * len(parts))), ctx.alloc(max(32, 32 * len(parts)))
            bufs += [b for b in (d_blob, d_stab, d_sscr, d_hit, d_stres, d_mres2) if b is not None]
            d_blob.upload(blob)
            d_stab.zero()
            if a.skip_retransmits or a.reassemble:
                qneed = abi.flow_tcpseq_scratch_bytes(max_n, cap)
                d_qtab, d_qscr, d_keep = ctx.alloc(128 * cap), ctx.alloc(max(256, qneed)), ctx.alloc(max(16, (max_n + 63) // 64 * 8))
                d_qres = ctx.alloc(max(64, 64 * len(parts)))
                bufs += [d_qtab, d_qscr, d_keep, d_qres]
                d_qtab.zero()
            if a.reassemble:
                rneed = abi.flow_reasm_scratch_bytes(max_n, cap)
                d_off, d_rtab, d_rscr = ctx.alloc(max(16, 8 * max_n)), ctx.alloc(128 * cap), ctx.alloc(max(256, rneed))
                d_rhit = ctx.alloc(max(16, (max_n + 63) // 64 * 8))
                d_rres, d_mres3 = ctx.alloc(max(64, 64 * len(parts))), ctx.alloc(max(32, 32 * len(parts)))
                bufs += [d_off, d_rtab, d_rscr, d_rhit, d_rres, d_mres3]
                d_rtab.zero()
        d_marks.zero()
        ctx.reserve(max_n)
        ctx.flow_track_init(d_state, lay["total"], cap, flags)

        def stage(lo, hi):
            n = hi - lo
            first = int(off[lo]) - LEAD   # the chunk starts at its first record's header
            size = int(off[hi - 1] + ln[hi - 1]) - first
            d_data.upload(data[first:first + size])   # waits for the context's stream: the last chunk is done
            d_desc.upload((off[lo:hi] - first).astype(np.uint64) | (ln[lo:hi].astype(np.uint64) << np.uint64(48)))
            return abi.Batch(d_data.ptr, d_desc.ptr, 0, n, size, abi.DESC_PACKED, 0)

        for k, (lo, hi) in enumerate(parts):   # pass one: the marks
            batch = stage(lo, hi)
            ver, ids = d_ver.ptr + 8 * int(word0[k]), d_ids.ptr + 4 * lo
            if filters:
                ctx.run_device(batch, abi.Outputs(None, 0, ver, None, None, None))
            ctx.flow_track_update(d_state, batch, d_scratch, need, d_res, flow_id=ids)
            if blob is not None:
                hit = d_hit.ptr if filters else ver
                keep = None
                if a.skip_retransmits:   # every packet but the old segments
                    keep = d_keep
                    ctx.flow_tcpseq(batch, ids, None, flags, d_qtab, cap, d_qscr, qneed, d_qres.ptr + 64 * k, out_select=d_keep)
                if a.reassemble:   # TCP in sequence order; what was not placed stays for the arrival-order matcher
                    keep = d_keep
                    ctx.flow_tcpseq(batch, ids, None, flags, d_qtab, cap, d_qscr, qneed, d_qres.ptr + 64 * k, off=d_off)
                    ctx.flow_reasm(batch, ids, None, d_off, flags, blob, d_blob, d_rtab, cap, d_rscr, rneed, d_rres.ptr + 64 * k,
                                   hit=d_rhit, rest=d_keep)
                    ctx.flow_mark_update(batch, ids, d_rhit, MARK, d_marks, cap, d_mres3.ptr + 32 * k)
                ctx.flow_stream(batch, ids, keep, flags, blob, d_blob, d_stab, cap, d_sscr, sneed, d_stres.ptr + 64 * k, hit=hit)
                ctx.flow_mark_update(batch, ids, hit, MARK, d_marks, cap, (d_mres2 if filters else d_mres).ptr + 32 * k)
            if filters:
                ctx.flow_mark_update(batch, ids, ver, MARK, d_marks, cap, d_mres.ptr + 32 * k)
        ctx.synchronize()
        hdr = abi.FlowTrackHdr.from_bytes(d_state.download(np.zeros(128, np.uint8))).as_dict()
        if hdr["overflow_packets"]:
            raise SystemExit(f"pcap_sessions: more than --flow-cap {cap} flows: a session would be incomplete, nothing is written")
        out["flows"] = hdr["n_flows"]
        if parts:
            raw = d_mres.download(np.zeros(32 * len(parts), np.uint8))
            for k in range(len(parts)):
                r = abi.FlowMarkResult.from_bytes(raw[32 * k:32 * k + 32]).as_dict()
                if r["bad_ids"]:
                    raise SystemExit("pcap_sessions: the tracker's flow ids do not fit the mark table")
                out["hit_packets"] += r["hit_packets"]
                out["marked_flows"] += r["new_marked_flows"]
                out["unkeyed_hits"] += r["unkeyed_hits"]
            if blob is not None:
                raw, raw2 = d_stres.download(np.zeros(64 * len(parts), np.uint8)), d_mres2.download(np.zeros(32 * len(parts), np.uint8))
                out.update(stream_packets=0, stream_bytes=0, stream_hit_packets=0)
                for k in range(len(parts)):
                    r = abi.FlowStreamResult.from_bytes(raw[64 * k:64 * k + 64]).as_dict()
                    if r["bad_ids"]:
                        raise SystemExit("pcap_sessions: the tracker's flow ids do not fit the stream table")
                    out["stream_packets"] += r["stream_packets"]
                    out["stream_bytes"] += r["stream_bytes"]
                    out["stream_hit_packets"] += r["hit_packets"]
                    if filters:   # the flows the stream's hits marked first
                        out["marked_flows"] += abi.FlowMarkResult.from_bytes(raw2[32 * k:32 * k + 32]).as_dict()["new_marked_flows"]
                if a.skip_retransmits or a.reassemble:
                    raw = d_qres.download(np.zeros(64 * len(parts), np.uint8))
                    out.update(seq_packets=0, old_packets=0)
                    for k in range(len(parts)):
                        r = abi.FlowTcpseqResult.from_bytes(raw[64 * k:64 * k + 64]).as_dict()
                        out["seq_packets"] += r["seq_packets"]
                        out["old_packets"] += r["old"]
                if a.reassemble:
                    raw, raw3 = d_rres.download(np.zeros(64 * len(parts), np.uint8)), d_mres3.download(np.zeros(32 * len(parts), np.uint8))
                    names = ("holes", "dup_packets", "late_packets", "far_packets")
                    out.update(reasm_packets=0, reasm_bytes=0, reasm_hit_packets=0, **{name: 0 for name in names})
                    for k in range(len(parts)):
                        r = abi.FlowReasmResult.from_bytes(raw[64 * k:64 * k + 64]).as_dict()
                        if r["bad_ids"]:
                            raise SystemExit("pcap_sessions: the tracker's flow ids do not fit the reassembly table")
                        out["reasm_packets"] += r["stream_packets"]
                        out["reasm_bytes"] += r["stream_bytes"]
                        out["reasm_hit_packets"] += r["hit_packets"]
                        for name in names:
                            out[name] += r[name]
                        # the flows the reassembly's hits marked first; its hit packets are reasm_hit_packets, as the stream's are stream_hit_packets
                        out["marked_flows"] += abi.FlowMarkResult.from_bytes(raw3[32 * k:32 * k + 32]).as_dict()["new_marked_flows"]
        if a.invert and parts:   # base = the packets that did not pass
            words = d_ver.download(np.zeros(8 * int(word0[-1]), np.uint8)).view(np.uint64)
            d_ver.upload(~words)
        fh = open(a.dst, "wb")
        fh.write(data[:24].tobytes())
        op = abi.FLOW_MARK_ANDNOT if a.invert else abi.FLOW_MARK_OR
        for k, (lo, hi) in enumerate(parts):   # pass two: the selection and the pack
            n = hi - lo
            batch = stage(lo, hi)
            ctx.flow_mark_select(d_ids.ptr + 4 * lo, n, d_marks, cap, MARK, d_sel, d_sres, op=op, base=d_ver.ptr + 8 * int(word0[k]))
            ctx.pass_pack(batch, d_sel, d_pack, d_pack.nbytes, d_tot, d_np, lead=LEAD)
            ctx.synchronize()
            total, count = int(d_tot.download(np.zeros(1, np.uint64))[0]), int(d_np.download(np.zeros(2, np.uint32))[0])
            sres = abi.FlowMarkSelectResult.from_bytes(d_sres.download(np.zeros(32, np.uint8))).as_dict()
            if total > d_pack.nbytes or count != sres["n_out"]:
                raise SystemExit("pcap_sessions: the pack disagrees with the selection")
            if total:
                fh.write(d_pack.download(np.zeros(total, np.uint8)).tobytes())   # only the packed bytes cross PCIe
            out["written_packets"] += count
            out["written_bytes"] += total - LEAD * count
        abi.Context.flow_track_forget(d_state)   # before its memory goes back
        for b in bufs:
            b.free()
        whole = True
    except abi.BtError as e:
        raise SystemExit(f"pcap_sessions: {e}")
    finally:
        if fh is not None:
            fh.close()
            if not whole:   # an error in pass two: no partial output stays behind
                os.remove(a.dst)
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

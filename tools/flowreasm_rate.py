"""The rate of per-flow TCP reassembly (bt_flow_tcpseq_device + bt_flow_reasm_device) against the chain it
extends, bt_flow_tcpseq_device + bt_flow_stream_device, on the bench's C3 capture on the device.

  reasm    bt_flow_reasm_device's kernels from the first one's start to the last one's end (events recorded by
           the kernels' own dispatches), hit and rest written, and what the time divides into: classification
           + compaction, the first sort (4 passes, by position), rekey + the second sort (by flow and
           direction), carry scan + join + emit, match, commit. The table is zeroed before every launch, so
           every launch places, sorts and matches every segment (into a table that has seen the call, every
           segment is late and the launch ends behind the classification: listed as late_ms). The offsets
           are those of a first bt_flow_tcpseq_device call.
  tcpseq   bt_flow_tcpseq_device with `off` written, in the same run: both chains begin with it
  stream   bt_flow_stream_device over the same packets, in the same run; rest_stream_ms is the same call over the
           reassembly's `rest` alone. chain_ms = tcpseq + reasm + the stream matcher on rest, the three calls
           tools/pcap_sessions.py --reassemble makes; parent_chain_ms = tcpseq + the stream matcher on everything
  Three id patterns: ids=tracker (the tracker's numbers; C3: every packet a flow of its own), ids=rr1024
  (1,024 flows round robin), ids=half_one (half the packets in one flow).

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches, all rounds
listed. Before anything is timed, hit, rest, the table and the result of a prefix of the batch are checked
against bt_flow_reasm_host, over two calls.
Usage: python tools/flowreasm_rate.py [--packets N] [--steps K] [--rounds R] [--pattern EXPR] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowreasm/flowreasm_rate.jsonl).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from beatrice_amd import abi, synth  # noqa: E402

PHASES = ("class_ms", "sort_pos_ms", "sort_key_ms", "scan_ms", "match_ms", "commit_ms")


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-packets", type=int, default=1 << 15)
    ap.add_argument("--pattern", default="GET|POST")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowreasm", "flowreasm_rate.jsonl"))
    a = ap.parse_args()
    lines = []

    def line(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def stats(r):
        return {"ms_median": round(med(r), 4), "ms_rounds": [round(x, 4) for x in sorted(r)]}

    ctx = abi.Context(0)
    L = abi.lib()
    try:
        blob, _ = abi.flow_stream_compile(a.pattern)
        d_blob = ctx.alloc(len(blob))
        d_blob.upload(blob)
        wl = bench.WORKLOADS["c3"]
        cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
        run, n = cap.run, cap.n
        nw = (n + 63) // 64
        ctx.reserve(n)
        one = (ctypes.c_float * 1)()
        ph6 = (ctypes.c_float * 6)()
        ms = (ctypes.c_float * a.steps)()
        d_id = ctx.alloc(4 * n)
        need = abi.flow_track_scratch_bytes(n)
        d_scratch, d_res = ctx.alloc(need), ctx.alloc(64)
        lay = abi.flow_track_layout(n)
        d_state = ctx.alloc(lay["total"])
        ctx.flow_track_init(d_state, lay["total"], n)
        ctx.flow_track_update(d_state, run.batch, d_scratch, need, d_res, batch_ts=7, flow_id=d_id)   # d_id: the flows' numbers
        ctx.synchronize()
        res = abi.FlowTrackResult.from_bytes(d_res.download(np.zeros(64, np.uint8))).as_dict()
        assert res["overflow_flows"] == 0 and res["status"] == 0
        nf = max(1, res["n_flows"])
        abi.Context.flow_track_forget(d_state)
        d_scratch.free()
        d_state.free()
        d_off, d_hit, d_rest, d_rres, d_qres, d_sres = ctx.alloc(8 * n), ctx.alloc(8 * nw), ctx.alloc(8 * nw), ctx.alloc(64), ctx.alloc(64), ctx.alloc(64)
        d_work = ctx.alloc(max(abi.flow_reasm_scratch_bytes(n, n), abi.flow_tcpseq_scratch_bytes(n, n), abi.flow_stream_scratch_bytes(n, n)))
        qouts = abi.FlowTcpseqOut(None, d_off.ptr, None, d_qres.ptr, (ctypes.c_uint64 * 2)(0, 0))
        routs = abi.FlowReasmOut(d_hit.ptr, d_rest.ptr, d_rres.ptr, (ctypes.c_uint64 * 2)(0, 0))
        souts = abi.FlowStreamOut(d_hit.ptr, d_sres.ptr, (ctypes.c_uint64 * 2)(0, 0))

        # right before it is timed: a prefix against the host forms, twice into the same tables
        m = min(n, a.check_packets)
        ids = d_id.download(np.zeros(m, np.uint32)) & np.uint32(255)   # 256 flows: long streams in the scan
        desc = np.ascontiguousarray(cap.desc[:m], np.uint64)
        end = int(((desc & np.uint64((1 << 48) - 1)) + (desc >> np.uint64(48))).max())
        nbytes = (end + 15) // 16 * 16
        data = run.d_data.download(np.zeros(nbytes, np.uint8))
        d_qtab, d_tab, d_cid = ctx.alloc(128 * 256), ctx.alloc(128 * 256), ctx.alloc(4 * m)
        d_qtab.zero()
        d_tab.zero()
        d_cid.upload(ids)
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, nbytes, run.batch.desc_format, 0)
        hq, host = np.zeros(256, abi.FlowTcpseqRec), np.zeros(256, abi.FlowReasmRec)
        for k in range(2):
            ctx.flow_tcpseq(pre, d_cid, None, 0, d_qtab, 256, d_work, abi.flow_tcpseq_scratch_bytes(m, 256), d_qres, off=d_off)
            ctx.flow_reasm(pre, d_cid, None, d_off, 0, blob, d_blob, d_tab, 256, d_work, abi.flow_reasm_scratch_bytes(m, 256), d_rres,
                           hit=d_hit, rest=d_rest)
            ctx.synchronize()
            hoff, hhit, hrest = np.zeros(m, np.int64), np.zeros((m + 63) // 64, np.uint64), np.zeros((m + 63) // 64, np.uint64)
            abi.flow_tcpseq_host(data, desc, ids, None, 0, hq, off=hoff)
            hres = abi.flow_reasm_host(data, desc, ids, None, hoff, 0, blob, host, hit=hhit, rest=hrest)
            assert abi.FlowReasmResult.from_bytes(d_rres.download(np.zeros(64, np.uint8))).as_dict() == hres, "the result differs from the host form"
            assert d_tab.download(np.zeros(128 * 256, np.uint8)).tobytes() == host.tobytes(), "the table differs from the host form"
            assert (d_hit.download(np.zeros((m + 63) // 64, np.uint64)) == hhit).all(), "hit differs from the host form"
            assert (d_rest.download(np.zeros((m + 63) // 64, np.uint64)) == hrest).all(), "rest differs from the host form"
        for b in (d_qtab, d_tab, d_cid):
            b.free()

        i = np.arange(n, dtype=np.uint32)
        half = np.where(i & 1, np.uint32(0), i).astype(np.uint32)
        variants = (("tracker", None, nf), ("rr1024", i & np.uint32(1023), 1024), ("half_one", half, n))
        for name, ids, flow_cap in variants:
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(np.ascontiguousarray(ids, np.uint32))
            d_qtab, d_tab, d_stab = ctx.alloc(128 * flow_cap), ctx.alloc(128 * flow_cap), ctx.alloc(32 * flow_cap)
            for b in (d_qtab, d_tab, d_stab):
                b.zero()
            qneed, rneed, sneed = abi.flow_tcpseq_scratch_bytes(n, flow_cap), abi.flow_reasm_scratch_bytes(n, flow_cap), abi.flow_stream_scratch_bytes(n, flow_cap)
            ctx.flow_tcpseq(run.batch, d_ids, None, 0, d_qtab, flow_cap, d_work, qneed, d_qres, off=d_off)   # the offsets of a first call
            ctx.synchronize()

            def reasm(fresh=True):
                if fresh:
                    d_tab.zero()
                    ctx.synchronize()
                abi._check(L.bt_time_flow_reasm(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, d_off.ptr, 0, blob.ctypes.data, d_blob.ptr,
                                                len(blob), d_tab.ptr, flow_cap, d_work.ptr, rneed, ctypes.byref(routs), 1, one, ph6))
                return one[0], list(ph6)

            def rround():
                got = [reasm() for _ in range(a.steps)]
                return med([g[0] for g in got]), [med([g[1][k] for g in got]) for k in range(6)]
            rround()
            rounds = [rround() for _ in range(a.rounds)]
            r = [x[0] for x in rounds]
            ph = [round(med([x[1][k] for x in rounds]), 4) for k in range(6)]
            t = abi.FlowReasmResult.from_bytes(d_rres.download(np.zeros(64, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["late_packets"] == 0
            late = med([reasm(False)[0] for _ in range(a.steps)])

            def tcpseq():
                abi._check(L.bt_time_flow_tcpseq(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, 0, d_qtab.ptr, flow_cap, d_work.ptr, qneed,
                                                 ctypes.byref(qouts), a.steps, ms, None))
                return med(list(ms))
            tcpseq()   # overwrites d_off: the reassembly was timed above
            q = stats([tcpseq() for _ in range(a.rounds)])

            def stream(select=None):
                abi._check(L.bt_time_flow_stream(ctx.h, ctypes.byref(run.batch), d_ids.ptr, select, 0, blob.ctypes.data, d_blob.ptr, len(blob),
                                                 d_stab.ptr, flow_cap, d_work.ptr, sneed, ctypes.byref(souts), a.steps, ms, None))
                return med(list(ms))
            stream(d_rest.ptr)   # what the reassembly did not place (UDP here), in arrival order: the chain's third call
            rest = stats([stream(d_rest.ptr) for _ in range(a.rounds)])
            d_stab.zero()
            stream()
            s = stats([stream() for _ in range(a.rounds)])
            both, parent = med(r) + q["ms_median"] + rest["ms_median"], s["ms_median"] + q["ms_median"]
            line(variant="reasm", ids=name, packets=n, flow_cap=flow_cap, pattern=a.pattern, stream_packets=t["stream_packets"],
                 stream_bytes=t["stream_bytes"], hit_packets=t["hit_packets"], holes=t["holes"], dup_packets=t["dup_packets"], **stats(r),
                 **dict(zip(PHASES, ph)), late_ms=round(late, 4), sort_pos_share=round(ph[1] / med(r), 3),
                 tcpseq_ms=q["ms_median"], rest_stream_ms=rest["ms_median"], stream_ms=s["ms_median"], chain_ms=round(both, 4), parent_chain_ms=round(parent, 4),
                 chain_ratio=round(both / parent, 3), reasm_to_stream=round(med(r) / s["ms_median"], 3),
                 gpps=round(n / (med(r) * 1e-3) / 1e9, 3))
            line(variant="tcpseq", ids=name, packets=n, flow_cap=flow_cap, **q)
            line(variant="stream", ids=name, packets=n, flow_cap=flow_cap, **s)
            for b in (d_qtab, d_tab, d_stab):
                b.free()
            if ids is not None:
                d_ids.free()

        for b in (d_id, d_res, d_off, d_hit, d_rest, d_rres, d_qres, d_sres, d_work, d_blob):
            b.free()
        run.free()
    finally:
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The rate of per-flow stream matching (bt_flow_stream_device) and of what it is measured against,
on the bench's C3 capture on the device.

  stream        the call's kernels from the first one's start to the last one's end (events recorded by
                the kernels' own dispatches), with the hit words written, and what the time divides
                into: classification + compaction, sort (every pass), link + match, commit. Pattern
                GET|POST (--pattern). Four id patterns:
                ids=tracker     the flow numbers bt_flow_track_update_device gave the capture (C3: every
                                packet a flow of its own)
                ids=rr1024      1,024 flows round robin
                ids=half_one    half the packets in one flow, the rest each in a flow of its own
                ids=tracker_c3  the tracker's ids, select = the c3 program's verdict
                The table is zero before the first call, which is listed apart.
  flowseq       bt_flow_seq_device on the tracker's ids, every output written, in the same run
  flowstat      bt_flow_stat_update_device on the tracker's ids, in the same run
  copy          one hipMemcpyAsync device-to-device of the batch's payload bytes (the result's
                stream_bytes): the floor of a pass that must read every payload byte

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the hit words, the table and the result of a prefix of
the batch are checked against bt_flow_stream_host.
Usage: python tools/flowstream_rate.py [--packets N] [--steps K] [--rounds R] [--pattern EXPR] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowstream/flowstream_rate.jsonl).
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


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-packets", type=int, default=1 << 16)
    ap.add_argument("--pattern", default="GET|POST")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowstream", "flowstream_rate.jsonl"))
    a = ap.parse_args()
    lines = []

    def line(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def stats(r):
        return {"ms_median": round(med(r), 4), "ms_rounds": [round(x, 4) for x in sorted(r)]}

    blob, info = abi.flow_stream_compile(a.pattern)
    ctx = abi.Context(0)
    L = abi.lib()
    try:
        wl = bench.WORKLOADS["c3"]
        cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
        run, n = cap.run, cap.n
        nw = (n + 63) // 64
        ctx.reserve(n)
        ctx.compile(wl["filters"])
        run.run()   # run.d_ver: the c3 program's verdict
        ms = (ctypes.c_float * a.steps)()
        phase = (ctypes.c_float * (4 * a.steps))()
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
        d_blob = ctx.alloc(len(blob))
        d_blob.upload(blob)
        d_hit, d_sres = ctx.alloc(8 * nw), ctx.alloc(64)
        d_work = ctx.alloc(max(abi.flow_stream_scratch_bytes(n, n), abi.flow_seq_scratch_bytes(n, n)))
        outs = abi.FlowStreamOut(d_hit.ptr, d_sres.ptr, (ctypes.c_uint64 * 2)(0, 0))

        # right before it is timed: a prefix against the host form, hit words, table and result
        m = min(n, a.check_packets)
        ids = d_id.download(np.zeros(m, np.uint32))
        desc = np.ascontiguousarray(cap.desc[:m], np.uint64)
        end = int(((desc & np.uint64((1 << 48) - 1)) + (desc >> np.uint64(48))).max())
        nbytes = (end + 15) // 16 * 16
        data = run.d_data.download(np.zeros(nbytes, np.uint8))
        d_tab = ctx.alloc(32 * nf)
        d_tab.zero()
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, nbytes, run.batch.desc_format, 0)
        ctx.flow_stream(pre, d_id, None, 0, blob, d_blob, d_tab, nf, d_work, abi.flow_stream_scratch_bytes(m, nf), d_sres, hit=d_hit)
        ctx.synchronize()
        host, hhit = np.zeros(nf, abi.FlowStreamRec), np.zeros((m + 63) // 64, np.uint64)
        hres = abi.flow_stream_host(data, desc, ids, None, 0, blob, host, hit=hhit)
        assert abi.FlowStreamResult.from_bytes(d_sres.download(np.zeros(64, np.uint8))).as_dict() == hres, "the result differs from the host form"
        assert d_tab.download(np.zeros(32 * nf, np.uint8)).tobytes() == host.tobytes(), "the table differs from the host form"
        assert (d_hit.download(np.zeros((m + 63) // 64, np.uint64)) == hhit).all(), "the hit words differ from the host form"
        assert hres["stream_packets"] > 0
        d_tab.free()

        i = np.arange(n, dtype=np.uint32)
        half = np.where(i & 1, np.uint32(0), i).astype(np.uint32)
        variants = (("tracker", None, nf, None), ("rr1024", i & np.uint32(1023), 1024, None), ("half_one", half, n, None),
                    ("tracker_c3", None, nf, run.d_ver))
        stream_bytes = 0
        for name, ids, flow_cap, d_sel in variants:
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(np.ascontiguousarray(ids, np.uint32))
            d_tab = ctx.alloc(32 * flow_cap)
            d_tab.zero()
            sneed = abi.flow_stream_scratch_bytes(n, flow_cap)

            def call():
                abi._check(L.bt_time_flow_stream(ctx.h, ctypes.byref(run.batch), d_ids.ptr, d_sel.ptr if d_sel else None, 0, blob.ctypes.data,
                                                 d_blob.ptr, len(blob), d_tab.ptr, flow_cap, d_work.ptr, sneed, ctypes.byref(outs), a.steps,
                                                 ms, phase))
                ph = np.array(list(phase), np.float64).reshape(a.steps, 4)
                return list(ms), [med(list(ph[:, k])) for k in range(4)]
            first, _ = call()   # the first call of it finds a zero table
            rounds = [call() for _ in range(a.rounds)]
            r = [med(x[0]) for x in rounds]
            ph = [round(med([x[1][k] for x in rounds]), 4) for k in range(4)]
            t = abi.FlowStreamResult.from_bytes(d_sres.download(np.zeros(64, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["stream_packets"] > 0
            if name == "tracker":
                stream_bytes = t["stream_bytes"]
            line(variant="stream", ids=name, pattern=a.pattern, positions=info["positions"], packets=n, flow_cap=flow_cap,
                 selected=t["selected"], stream_packets=t["stream_packets"], stream_bytes=t["stream_bytes"], hit_packets=t["hit_packets"],
                 first_call_ms=round(first[0], 4), **stats(r), class_ms=ph[0], sort_ms=ph[1], match_ms=ph[2], commit_ms=ph[3],
                 gpps=round(n / (med(r) * 1e-3) / 1e9, 3), payload_gbps=round(t["stream_bytes"] / (med(r) * 1e-3) / 1e9, 1))
            d_tab.free()
            if ids is not None:
                d_ids.free()

        d_seq, d_off, d_out, d_qres = ctx.alloc(4 * n), ctx.alloc(8 * n), ctx.alloc(8 * nw), ctx.alloc(64)
        d_qtab = ctx.alloc(16 * nf)
        d_qtab.zero()
        qopts = abi.FlowSeqOpts(0, 0, abi.FLOW_SEQ_KEEP_UNKEYED, (ctypes.c_uint32 * 3)(0, 0, 0))
        qouts = abi.FlowSeqOut(d_seq.ptr, d_off.ptr, d_out.ptr)
        qneed = abi.flow_seq_scratch_bytes(n, nf)

        def seq():
            abi._check(L.bt_time_flow_seq(ctx.h, ctypes.byref(run.batch), d_id.ptr, None, ctypes.byref(qopts), d_qtab.ptr, nf,
                                          ctypes.byref(qouts), d_work.ptr, qneed, d_qres.ptr, a.steps, ms, None))
            return med(list(ms))
        seq()
        line(variant="flowseq", ids="tracker", packets=n, flow_cap=nf, **stats([seq() for _ in range(a.rounds)]))

        d_stat, d_tres = ctx.alloc(128 * nf), ctx.alloc(32)
        d_stat.zero()
        upd = abi.FlowTrackUpdate(None, 7)

        def stat():
            abi._check(L.bt_time_flow_stat(ctx.h, ctypes.byref(run.batch), d_id.ptr, 0, ctypes.byref(upd), d_stat.ptr, nf, d_tres.ptr,
                                           a.steps, ms))
            return med(list(ms))
        stat()
        line(variant="flowstat", ids="tracker", packets=n, flow_cap=nf, **stats([stat() for _ in range(a.rounds)]))

        moved = max(16, stream_bytes)
        d_src, d_dst = ctx.alloc(moved + 256), ctx.alloc(moved + 256)

        def copy():
            abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_src.ptr, moved, a.steps, ms))
            return med(list(ms))
        copy()
        r = stats([copy() for _ in range(a.rounds)])
        line(variant="copy", bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)
        for b in (d_id, d_res, d_blob, d_hit, d_sres, d_work, d_seq, d_off, d_out, d_qres, d_qtab, d_stat, d_tres, d_src, d_dst):
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

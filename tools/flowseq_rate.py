"""The rate of the per-flow numbering and cut-off (bt_flow_seq_device) and of what it is measured
against, on the bench's C3 capture on the device.

  seq           the call's kernels from the first one's start to the last one's end (events recorded by
                the kernels' own dispatches), with seq, byte_off and out_select written and no limit (every
                numbered packet is kept: a keep bit per packet, the emit's dearest case), and what the
                time divides into: compaction, sort (every pass, and per pass), segmented scan, emit +
                table update. Five id patterns, and the first again behind its cut-off:
                ids=tracker     the flow numbers bt_flow_track_update_device gave the capture
                ids=one         every packet in flow 0 (flow_cap = 1: no sort pass)
                ids=rr1024      1,024 flows round robin
                ids=skewed      half the packets in one flow, the rest over 5,000 flows
                ids=tracker_c3  the tracker's ids, select = the c3 program's verdict
                ids=tracker_cut the tracker's ids with max_packets = 3: from the fourth call on no packet is kept
                The table is zero before the first call, which is listed apart.
  flowmark      bt_flow_mark_update_device with every packet a hit, on the tracker's ids, in the same run
  copy          one hipMemcpyAsync device-to-device of n * 4 bytes
  host          bt_flow_seq_host on one thread over the first --host-packets packets (tracker ids)

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the outputs, the table and the result of a prefix of
the batch are checked against bt_flow_seq_host.
Usage: python tools/flowseq_rate.py [--packets N] [--steps K] [--rounds R] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowseq/flowseq_rate.jsonl).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from beatrice_amd import abi, synth  # noqa: E402


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def passes_of(flow_cap):
    return 0 if flow_cap <= 1 else ((flow_cap - 1).bit_length() + 7) // 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-packets", type=int, default=1 << 18)
    ap.add_argument("--host-packets", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowseq", "flowseq_rate.jsonl"))
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
        d_seq, d_off, d_out, d_sres = ctx.alloc(4 * n), ctx.alloc(8 * n), ctx.alloc(8 * nw), ctx.alloc(64)
        no_limit = abi.FlowSeqOpts(0, 0, abi.FLOW_SEQ_KEEP_UNKEYED, (ctypes.c_uint32 * 3)(0, 0, 0))
        first_three = abi.FlowSeqOpts(3, 0, abi.FLOW_SEQ_KEEP_UNKEYED, (ctypes.c_uint32 * 3)(0, 0, 0))
        outs = abi.FlowSeqOut(d_seq.ptr, d_off.ptr, d_out.ptr)
        seq_need = abi.flow_seq_scratch_bytes(n, n)
        d_work = ctx.alloc(seq_need)

        # right before it is timed: a prefix against the host form, outputs, table and result
        m = min(n, a.check_packets)
        ids = d_id.download(np.zeros(m, np.uint32))
        ver = run.d_ver.download(np.zeros((m + 63) // 64, np.uint64))
        d_tab = ctx.alloc(16 * nf)
        d_tab.zero()
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, run.batch.bytes, run.batch.desc_format, 0)
        ctx.flow_seq(pre, d_id, run.d_ver, d_tab, nf, d_work, seq_need, d_sres, max_packets=3, flags=abi.FLOW_SEQ_KEEP_UNKEYED,
                     seq=d_seq, byte_off=d_off, out_select=d_out)
        ctx.synchronize()
        host = np.zeros(nf, abi.FlowSeqRec)
        hseq, hoff, hout = np.zeros(m, np.uint32), np.zeros(m, np.uint64), np.zeros((m + 63) // 64, np.uint64)
        hres = abi.flow_seq_host(cap.desc[:m], ids, ver, host, 3, 0, abi.FLOW_SEQ_KEEP_UNKEYED, seq=hseq, byte_off=hoff, out_select=hout)
        assert abi.FlowSeqResult.from_bytes(d_sres.download(np.zeros(64, np.uint8))).as_dict() == hres, "the result differs from the host form"
        assert d_tab.download(np.zeros(16 * nf, np.uint8)).tobytes() == host.tobytes(), "the table differs from the host form"
        assert (d_seq.download(np.zeros(m, np.uint32)) == hseq).all() and (d_off.download(np.zeros(m, np.uint64)) == hoff).all()
        assert (d_out.download(np.zeros((m + 63) // 64, np.uint64)) == hout).all(), "the kept words differ from the host form"
        assert hres["numbered"] > 0
        d_tab.free()

        rng = np.random.default_rng(1)
        skew = np.where(rng.integers(0, 2, n) == 0, 5000, rng.integers(0, 5000, n)).astype(np.uint32)
        variants = (("tracker", None, nf, None, no_limit), ("one", np.zeros(n, np.uint32), 1, None, no_limit),
                    ("rr1024", (np.arange(n, dtype=np.uint32) & 1023), 1024, None, no_limit), ("skewed", skew, 5001, None, no_limit),
                    ("tracker_c3", None, nf, run.d_ver, no_limit), ("tracker_cut", None, nf, None, first_three))
        for name, ids, flow_cap, d_sel, opts in variants:
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(np.ascontiguousarray(ids, np.uint32))
            d_tab = ctx.alloc(16 * flow_cap)
            d_tab.zero()
            sneed = abi.flow_seq_scratch_bytes(n, flow_cap)

            def call():
                abi._check(L.bt_time_flow_seq(ctx.h, ctypes.byref(run.batch), d_ids.ptr, d_sel.ptr if d_sel else None, ctypes.byref(opts),
                                              d_tab.ptr, flow_cap, ctypes.byref(outs), d_work.ptr, sneed, d_sres.ptr, a.steps, ms, phase))
                ph = np.array(list(phase), np.float64).reshape(a.steps, 4)
                return list(ms), [med(list(ph[:, k])) for k in range(4)]
            first, _ = call()   # the first call of it finds a zero table (with max_packets = 3 the first three of it keep packets)
            rounds = [call() for _ in range(a.rounds)]
            r = [med(x[0]) for x in rounds]
            ph = [round(med([x[1][k] for x in rounds]), 4) for k in range(4)]
            t = abi.FlowSeqResult.from_bytes(d_sres.download(np.zeros(64, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["numbered"] > 0 and t["new_flows"] == 0
            assert t["kept"] == (0 if opts is first_three else t["numbered"] + t["unkeyed"])
            np_ = passes_of(flow_cap)
            line(variant="seq", ids=name, packets=n, flow_cap=flow_cap, selected=t["selected"], numbered=t["numbered"], flows=t["flows"],
                 kept=t["kept"], first_call_ms=round(first[0], 4), **stats(r), compact_ms=ph[0], sort_ms=ph[1], sort_passes=np_,
                 sort_pass_ms=round(ph[1] / np_, 4) if np_ else 0.0, scan_ms=ph[2], emit_ms=ph[3],
                 gpps=round(n / (med(r) * 1e-3) / 1e9, 3))
            d_tab.free()
            if ids is not None:
                d_ids.free()

        d_marks, d_mres = ctx.alloc(32 * nf), ctx.alloc(32)
        d_marks.zero()
        upd = abi.FlowMarkUpdate(1, 0, None, 7)

        def mark_update():
            abi._check(L.bt_time_flow_mark(ctx.h, ctypes.byref(run.batch), d_id.ptr, None, ctypes.byref(upd), d_marks.ptr, nf, d_mres.ptr,
                                           None, None, None, None, a.steps, ms, None))
            return list(ms)
        first = mark_update()
        r = [med(mark_update()) for _ in range(a.rounds)]
        line(variant="flowmark", hits="all", ids="tracker", packets=n, flow_cap=nf, first_call_ms=round(first[0], 4), **stats(r),
             gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
        moved = 4 * n
        d_dst = ctx.alloc(moved + 256)

        def copy():
            abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_id.ptr, moved, a.steps, ms))
            return med(list(ms))
        copy()
        r = stats([copy() for _ in range(a.rounds)])
        line(variant="copy", bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)

        hm = min(n, a.host_packets)
        ids = d_id.download(np.zeros(hm, np.uint32))
        host = np.zeros(nf, abi.FlowSeqRec)
        hseq, hoff, hout = np.zeros(hm, np.uint32), np.zeros(hm, np.uint64), np.zeros((hm + 63) // 64, np.uint64)
        desc = np.ascontiguousarray(cap.desc[:hm], np.uint64)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            abi.flow_seq_host(desc, ids, None, host, 3, 0, abi.FLOW_SEQ_KEEP_UNKEYED, seq=hseq, byte_off=hoff, out_select=hout)
            times.append((time.perf_counter() - t0) * 1e3)
        line(variant="host", ids="tracker", packets=hm, threads=1, **stats(times), gpps=round(hm / (med(times) * 1e-3) / 1e9, 4))
        for b in (d_id, d_res, d_seq, d_off, d_out, d_sres, d_work, d_marks, d_mres, d_dst):
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

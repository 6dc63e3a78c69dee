"""The rate of the per-flow TCP sequence classification (bt_flow_tcpseq_device) and of what it is
measured against, on the bench's C3 capture on the device.

  tcpseq        the call's kernels from the first one's start to the last one's end (events recorded by
                the kernels' own dispatches), every output written, and what the time divides into:
                classification + compaction, sort (every pass), carry scan + join, emit + commit.
                Three id patterns:
                ids=tracker     the flow numbers bt_flow_track_update_device gave the capture (C3: every
                                packet a flow of its own)
                ids=rr1024      1,024 flows round robin
                ids=half_one    half the packets in one flow, the rest each in a flow of its own
                The table is zero before the first call, which is listed apart; from the second call on
                every segment lies at or below what the first one saw (old), which is the case with the
                most work in the emit: every packet clears its bit in out_select.
  flowseq       bt_flow_seq_device on the same ids, every output written, in the same run: the yardstick
                (the same sort, the same scan shape, no frame byte read); ratio = tcpseq / flowseq
  flowstat      bt_flow_stat_update_device on the same ids, in the same run

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the classes, the offsets, the selection, the table and
the result of a prefix of the batch are checked against bt_flow_tcpseq_host, over two calls.
Usage: python tools/flowtcpseq_rate.py [--packets N] [--steps K] [--rounds R] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowtcpseq/flowtcpseq_rate.jsonl).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowtcpseq", "flowtcpseq_rate.jsonl"))
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
        d_cls, d_off, d_out, d_sres = ctx.alloc(n), ctx.alloc(8 * n), ctx.alloc(8 * nw), ctx.alloc(64)
        d_work = ctx.alloc(max(abi.flow_tcpseq_scratch_bytes(n, n), abi.flow_seq_scratch_bytes(n, n)))
        outs = abi.FlowTcpseqOut(d_cls.ptr, d_off.ptr, d_out.ptr, d_sres.ptr, (ctypes.c_uint64 * 2)(0, 0))

        # right before it is timed: a prefix against the host form, twice into the same table
        m = min(n, a.check_packets)
        ids = d_id.download(np.zeros(m, np.uint32)) & np.uint32(255)   # 256 flows: long segments in the scan
        desc = np.ascontiguousarray(cap.desc[:m], np.uint64)
        end = int(((desc & np.uint64((1 << 48) - 1)) + (desc >> np.uint64(48))).max())
        nbytes = (end + 15) // 16 * 16
        data = run.d_data.download(np.zeros(nbytes, np.uint8))
        d_tab, d_cid = ctx.alloc(128 * 256), ctx.alloc(4 * m)
        d_tab.zero()
        d_cid.upload(ids)
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, nbytes, run.batch.desc_format, 0)
        host = np.zeros(256, abi.FlowTcpseqRec)
        for k in range(2):
            ctx.flow_tcpseq(pre, d_cid, None, 0, d_tab, 256, d_work, abi.flow_tcpseq_scratch_bytes(m, 256), d_sres, cls=d_cls, off=d_off,
                            out_select=d_out)
            ctx.synchronize()
            hcls, hoff, hsel = np.zeros(m, np.uint8), np.zeros(m, np.int64), np.zeros((m + 63) // 64, np.uint64)
            hres = abi.flow_tcpseq_host(data, desc, ids, None, 0, host, cls=hcls, off=hoff, out_select=hsel)
            assert abi.FlowTcpseqResult.from_bytes(d_sres.download(np.zeros(64, np.uint8))).as_dict() == hres, "the result differs from the host form"
            assert d_tab.download(np.zeros(128 * 256, np.uint8)).tobytes() == host.tobytes(), "the table differs from the host form"
            assert (d_cls.download(np.zeros(m, np.uint8)) == hcls).all(), "the classes differ from the host form"
            assert (d_off.download(np.zeros(m, np.int64)) == hoff).all(), "the offsets differ from the host form"
            assert (d_out.download(np.zeros((m + 63) // 64, np.uint64)) == hsel).all(), "out_select differs from the host form"
            assert hres["seq_packets"] > 0
        d_tab.free()
        d_cid.free()

        d_seq, d_boff, d_qout, d_qres = ctx.alloc(4 * n), ctx.alloc(8 * n), ctx.alloc(8 * nw), ctx.alloc(64)
        qopts = abi.FlowSeqOpts(0, 0, abi.FLOW_SEQ_KEEP_UNKEYED, (ctypes.c_uint32 * 3)(0, 0, 0))
        qouts = abi.FlowSeqOut(d_seq.ptr, d_boff.ptr, d_qout.ptr)
        d_tres = ctx.alloc(32)
        upd = abi.FlowTrackUpdate(None, 7)

        i = np.arange(n, dtype=np.uint32)
        half = np.where(i & 1, np.uint32(0), i).astype(np.uint32)
        variants = (("tracker", None, nf), ("rr1024", i & np.uint32(1023), 1024), ("half_one", half, n))
        for name, ids, flow_cap in variants:
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(np.ascontiguousarray(ids, np.uint32))
            d_tab = ctx.alloc(128 * flow_cap)
            d_tab.zero()
            sneed = abi.flow_tcpseq_scratch_bytes(n, flow_cap)

            def call():
                abi._check(L.bt_time_flow_tcpseq(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, 0, d_tab.ptr, flow_cap, d_work.ptr, sneed,
                                                 ctypes.byref(outs), a.steps, ms, phase))
                ph = np.array(list(phase), np.float64).reshape(a.steps, 4)
                return list(ms), [med(list(ph[:, k])) for k in range(4)]
            first, _ = call()   # the first call of it finds a zero table
            rounds = [call() for _ in range(a.rounds)]
            r = [med(x[0]) for x in rounds]
            ph = [round(med([x[1][k] for x in rounds]), 4) for k in range(4)]
            t = abi.FlowTcpseqResult.from_bytes(d_sres.download(np.zeros(64, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["seq_packets"] > 0
            d_tab.free()

            d_qtab = ctx.alloc(16 * flow_cap)
            d_qtab.zero()
            qneed = abi.flow_seq_scratch_bytes(n, flow_cap)

            def seq():
                abi._check(L.bt_time_flow_seq(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, ctypes.byref(qopts), d_qtab.ptr, flow_cap,
                                              ctypes.byref(qouts), d_work.ptr, qneed, d_qres.ptr, a.steps, ms, None))
                return med(list(ms))
            seq()
            q = stats([seq() for _ in range(a.rounds)])
            d_qtab.free()
            line(variant="tcpseq", ids=name, packets=n, flow_cap=flow_cap, selected=t["selected"], seq_packets=t["seq_packets"],
                 seq_bytes=t["seq_bytes"], old=t["old"], first_call_ms=round(first[0], 4), **stats(r), class_ms=ph[0], sort_ms=ph[1],
                 scan_ms=ph[2], emit_ms=ph[3], gpps=round(n / (med(r) * 1e-3) / 1e9, 3), flowseq_ms=q["ms_median"],
                 ratio_to_flowseq=round(med(r) / q["ms_median"], 3))
            line(variant="flowseq", ids=name, packets=n, flow_cap=flow_cap, **q)

            d_stat = ctx.alloc(128 * flow_cap)
            d_stat.zero()

            def stat():
                abi._check(L.bt_time_flow_stat(ctx.h, ctypes.byref(run.batch), d_ids.ptr, 0, ctypes.byref(upd), d_stat.ptr, flow_cap,
                                               d_tres.ptr, a.steps, ms))
                return med(list(ms))
            stat()
            line(variant="flowstat", ids=name, packets=n, flow_cap=flow_cap, **stats([stat() for _ in range(a.rounds)]))
            d_stat.free()
            if ids is not None:
                d_ids.free()

        for b in (d_id, d_res, d_cls, d_off, d_out, d_sres, d_work, d_seq, d_boff, d_qout, d_qres, d_tres):
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

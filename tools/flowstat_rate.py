"""The rate of the statistics side table's update (bt_flow_stat_update_device) and of what it is
measured against, on the bench's C3 capture on the device, every packet selected.

  flowstat      the update's kernel between an event pair recorded by its own dispatch, on three id streams:
                ids=tracker   the flow numbers bt_flow_track_update_device gave the batch
                ids=one       every packet numbered 0: a batch that is one flow (flow_cap = 1)
                ids=distinct  packet i numbered i: every packet its own flow (flow_cap = n)
                The table is zero before the first call, which is listed apart; the timed calls find
                every OR and maximum in place (no atomicOr / atomicMax) and still add the sums.
  flowtcp       bt_flow_tcp_update_device on the same batch and the same three id streams, in the same
                run: the yardstick
  copy          one hipMemcpyAsync device-to-device of the batch's frame bytes

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the side table of a prefix of the batch is checked
against bt_flow_stat_update_host.
Usage: python tools/flowstat_rate.py [--packets N] [--steps K] [--rounds R] [--only STREAM] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowstat/flowstat_rate.jsonl).
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
    ap.add_argument("--check-packets", type=int, default=1 << 18)
    ap.add_argument("--only", default=None, help="one id stream alone, the statistics update only (a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowstat", "flowstat_rate.jsonl"))
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
        ctx.reserve(n)
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
        d_sres = ctx.alloc(32)
        upd = abi.FlowTrackUpdate(None, 7)
        # right before it is timed: a prefix against the host form, table and result
        m = min(n, a.check_packets)
        desc = cap.desc[:m]
        end = int(synth.desc_off(desc)[-1] + synth.desc_len(desc)[-1])
        frames = run.d_data.download(np.zeros(end, np.uint8))
        ids = d_id.download(np.zeros(m, np.uint32))
        d_stat = ctx.alloc(128 * nf)
        d_stat.zero()
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, run.batch.bytes, run.batch.desc_format, 0)
        ctx.flow_stat_update(pre, d_id, 0, d_stat, nf, d_sres, batch_ts=7)
        ctx.synchronize()
        host = np.zeros(nf, abi.FlowStatRec)
        hres = abi.flow_stat_update_host(frames, desc, ids, 0, host, batch_ts=7)
        assert abi.FlowStatResult.from_bytes(d_sres.download(np.zeros(32, np.uint8))).as_dict() == hres, "the update differs from the host form"
        assert d_stat.download(np.zeros(128 * nf, np.uint8)).tobytes() == host.tobytes(), "the side table differs from the host form"
        d_stat.free()

        streams = (("tracker", None, n), ("one", np.zeros(n, np.uint32), 1), ("distinct", np.arange(n, dtype=np.uint32), n))
        for name, ids, flow_cap in streams:
            if a.only and a.only != name:
                continue
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(ids)
            d_stat, d_tcp = ctx.alloc(128 * flow_cap), ctx.alloc(16 * flow_cap)
            d_stat.zero()
            d_tcp.zero()

            def stat_update():
                abi._check(L.bt_time_flow_stat(ctx.h, ctypes.byref(run.batch), d_ids.ptr, 0, ctypes.byref(upd), d_stat.ptr, flow_cap,
                                               d_sres.ptr, a.steps, ms))
                return list(ms)

            def tcp_update():
                abi._check(L.bt_time_flow_tcp(ctx.h, ctypes.byref(run.batch), d_ids.ptr, 0, d_tcp.ptr, flow_cap, d_sres.ptr, a.steps, ms))
                return list(ms)
            first = stat_update()   # the first call of it sets the ORs and the maxima
            r = [med(stat_update()) for _ in range(a.rounds)]
            t = abi.FlowStatResult.from_bytes(d_sres.download(np.zeros(32, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["ip_packets"] > 0
            line(variant="flowstat", ids=name, packets=n, flow_cap=flow_cap, ip_packets=t["ip_packets"], l4_packets=t["l4_packets"],
                 tcp_packets=t["tcp_packets"], first_call_ms=round(first[0], 4), **stats(r), gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
            if not a.only:
                first = tcp_update()
                r = [med(tcp_update()) for _ in range(a.rounds)]
                line(variant="flowtcp", ids=name, packets=n, flow_cap=flow_cap, first_call_ms=round(first[0], 4), **stats(r),
                     gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
            d_stat.free()
            d_tcp.free()
            if ids is not None:
                d_ids.free()
        if not a.only:
            moved = int(run.batch.bytes)
            d_dst = ctx.alloc(moved + 256)

            def copy():
                abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, run.batch.base, moved, a.steps, ms))
                return med(list(ms))
            copy()
            r = stats([copy() for _ in range(a.rounds)])
            line(variant="copy", bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)
            d_dst.free()
        abi.Context.flow_track_forget(d_state)
        for b in (d_id, d_scratch, d_res, d_state, d_sres):
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

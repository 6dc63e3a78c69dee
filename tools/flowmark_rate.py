"""The rate of the mark side table's update (bt_flow_mark_update_device) and of the selection built
from it (bt_flow_mark_select_device), and of what they are measured against, on the bench's C3
capture on the device with the flow numbers bt_flow_track_update_device gave it.

  update        the update's kernel between an event pair recorded by its own dispatch, on five hit sets:
                hits=none      hit words all zero: the kernel reads n / 8 bytes
                hits=1pct      one packet in a hundred, at random
                hits=all       every packet (hit = NULL)
                hits=all_one   every packet, every packet numbered 0: a batch that is one flow (flow_cap = 1)
                hits=all_own   every packet, packet i numbered i: every packet its own flow (flow_cap = n)
                The table is zero before the first call, which is listed apart; the timed calls find
                the mark and the stamps in place (no atomicOr / atomicMax) and still add the sums.
  select        the selection's kernel over the table the 1pct update left: op=SET, and op=OR with the
                1pct words as base
  flowtcp       bt_flow_tcp_update_device on the same batch and the tracker's ids, in the same run: the
                sibling that also reads frames
  copy          one hipMemcpyAsync device-to-device of n * 4 bytes: the selection's floor, it must read the ids
  checks        what the design promises: the update without hits takes less time than that copy, and the
                one-flow update is not slower than the update of distinct flows

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the table and the words of a prefix of the batch are
checked against bt_flow_mark_update_host / bt_flow_mark_select_host.
Usage: python tools/flowmark_rate.py [--packets N] [--steps K] [--rounds R] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowmark/flowmark_rate.jsonl).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowmark", "flowmark_rate.jsonl"))
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
        d_mres, d_sres, d_tres = ctx.alloc(32), ctx.alloc(32), ctx.alloc(32)
        rng = np.random.default_rng(1)
        pct = np.packbits(rng.random(nw * 64) < 0.01, bitorder="little").view(np.uint64)
        d_zero, d_pct, d_out = ctx.alloc(8 * nw), ctx.alloc(8 * nw), ctx.alloc(8 * nw)
        d_zero.zero()
        d_pct.upload(pct)
        upd = abi.FlowMarkUpdate(1, 0, None, 7)
        # right before it is timed: a prefix against the host forms, table, words and results
        m = min(n, a.check_packets)
        desc = cap.desc[:m]
        ids = d_id.download(np.zeros(m, np.uint32))
        d_marks = ctx.alloc(32 * nf)
        d_marks.zero()
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, run.batch.bytes, run.batch.desc_format, 0)
        ctx.flow_mark_update(pre, d_id, d_pct, 1, d_marks, nf, d_mres, batch_ts=7)
        ctx.flow_mark_select(d_id, m, d_marks, nf, 1, d_out, d_sres, op=abi.FLOW_MARK_OR, base=d_pct)
        ctx.synchronize()
        host = np.zeros(nf, abi.FlowMarkRec)
        hres = abi.flow_mark_update_host(desc, ids, pct, 1, host, batch_ts=7)
        assert abi.FlowMarkResult.from_bytes(d_mres.download(np.zeros(32, np.uint8))).as_dict() == hres, "the update differs from the host form"
        assert d_marks.download(np.zeros(32 * nf, np.uint8)).tobytes() == host.tobytes(), "the mark table differs from the host form"
        hout, hsel = abi.flow_mark_select_host(ids, host, 1, abi.FLOW_MARK_OR, base=pct)
        assert abi.FlowMarkSelectResult.from_bytes(d_sres.download(np.zeros(32, np.uint8))).as_dict() == hsel, "the selection differs from the host form"
        assert (d_out.download(np.zeros((m + 63) // 64, np.uint64)) == hout).all(), "the selected words differ from the host form"
        assert hsel["n_out"] >= hsel["n_marked"] >= hres["marked_packets"] > 0, (hsel, hres)
        d_marks.free()

        opts = abi.FlowMarkSelectOpts(1, 0, abi.FLOW_MARK_SET, 0)
        medians = {}
        hitsets = (("none", d_zero, None, nf), ("1pct", d_pct, None, nf), ("all", None, None, nf),
                   ("all_one", None, np.zeros(n, np.uint32), 1), ("all_own", None, np.arange(n, dtype=np.uint32), n))
        for name, d_hit, ids, flow_cap in hitsets:
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(ids)
            d_marks = ctx.alloc(32 * flow_cap)
            d_marks.zero()

            def mark_update():
                abi._check(L.bt_time_flow_mark(ctx.h, ctypes.byref(run.batch), d_ids.ptr, d_hit.ptr if d_hit else None, ctypes.byref(upd),
                                               d_marks.ptr, flow_cap, d_mres.ptr, None, None, None, None, a.steps, ms, None))
                return list(ms)

            def select(op, base):
                opts.op = op
                abi._check(L.bt_time_flow_mark(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, None, d_marks.ptr, flow_cap, None,
                                               ctypes.byref(opts), base, d_out.ptr, d_sres.ptr, a.steps, None, ms))
                return list(ms)
            first = mark_update()   # the first call of it sets the mark and the stamps
            r = [med(mark_update()) for _ in range(a.rounds)]
            t = abi.FlowMarkResult.from_bytes(d_mres.download(np.zeros(32, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["new_marked_flows"] == 0 and (t["hit_packets"] > 0) == (name != "none")
            medians[name] = med(r)
            line(variant="update", hits=name, packets=n, flow_cap=flow_cap, hit_packets=t["hit_packets"], marked_packets=t["marked_packets"],
                 unkeyed_hits=t["unkeyed_hits"], first_call_ms=round(first[0], 4), **stats(r), gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
            if name == "1pct":   # the selection over a table in which some flows are marked
                for op, base, label in ((abi.FLOW_MARK_SET, None, "SET"), (abi.FLOW_MARK_OR, d_pct.ptr, "OR")):
                    select(op, base)
                    r = [med(select(op, base)) for _ in range(a.rounds)]
                    s = abi.FlowMarkSelectResult.from_bytes(d_sres.download(np.zeros(32, np.uint8))).as_dict()
                    assert s["n"] == n and s["bad_ids"] == 0 and s["n_out"] >= s["n_marked"] > 0
                    line(variant="select", op=label, packets=n, n_marked=s["n_marked"], n_out=s["n_out"], **stats(r),
                         gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
            d_marks.free()
            if ids is not None:
                d_ids.free()
        d_tcp = ctx.alloc(16 * nf)
        d_tcp.zero()

        def tcp_update():
            abi._check(L.bt_time_flow_tcp(ctx.h, ctypes.byref(run.batch), d_id.ptr, 0, d_tcp.ptr, nf, d_tres.ptr, a.steps, ms))
            return list(ms)
        first = tcp_update()
        r = [med(tcp_update()) for _ in range(a.rounds)]
        line(variant="flowtcp", ids="tracker", packets=n, flow_cap=nf, first_call_ms=round(first[0], 4), **stats(r),
             gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
        moved = 4 * n
        d_dst = ctx.alloc(moved + 256)

        def copy():
            abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_id.ptr, moved, a.steps, ms))
            return med(list(ms))
        copy()
        r = stats([copy() for _ in range(a.rounds)])
        line(variant="copy", bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)
        line(variant="checks", no_hits_below_the_copy=bool(medians["none"] < r["ms_median"]),
             one_flow_not_slower_than_distinct=bool(medians["all_one"] <= medians["all_own"]))
        abi.Context.flow_track_forget(d_state)
        for b in (d_id, d_scratch, d_res, d_state, d_mres, d_sres, d_tres, d_zero, d_pct, d_out, d_tcp, d_dst):
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

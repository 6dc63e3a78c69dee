"""The rate of the top-K query over a flow tracker (bt_flow_track_top_device) and of what it replaces,
on trackers built from the bench's C3 capture on the device: once with every packet selected (every
packet its own flow) and once with the `c3` program's verdict words as `select`.

  flowtop       the query's kernels between an event pair recorded by the first and the last kernel's
                own dispatches, k = 1, 20, 4096, on three value sets:
                values=c3       metric bytes over the tracker as the capture left it
                values=random   metric bytes after the records were replaced by ones with random
                                full-width byte counts (the header stays)
                values=equal    metric packets over those records: every value is 0
  host          what the query replaces (bt_time_flow_top_host): the device-to-host copy of n_flows
                records into pinned memory, then a std::partial_sort for the first k on one thread
  copy          one hipMemcpyAsync device-to-device of n_flows x 104 bytes: the bytes the query must
                read once

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before a value set is timed its result is checked: total against the tracker's
header (c3) or numpy (random), top_total against the host baseline's own selection (c3), the
threshold against np.partition (random), and the all-equal top is flows 0 .. k-1.
Usage: python tools/flowtop_rate.py [--packets N] [--steps K] [--rounds R] [--select all|verdict] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowtop/flowtop_rate.jsonl).
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

KS = (1, 20, 4096)


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--select", choices=("all", "verdict"), default=None, help="one tracker alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowtop", "flowtop_rate.jsonl"))
    a = ap.parse_args()
    lines, failed = [], []

    def expect(ok, what):
        if not ok:
            failed.append(what)
            print("CHECK FAILED: " + what, file=sys.stderr, flush=True)

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
        ctx.compile(wl["filters"])
        ctx.reserve(n)
        ctx.run_device(run.batch, run.outs)   # verdict words
        ctx.synchronize()
        ms = (ctypes.c_float * a.steps)()
        need = abi.flow_track_scratch_bytes(n)
        d_scratch, d_res = ctx.alloc(need), ctx.alloc(64)
        for sel_name, sel in (("all", None), ("verdict", run.d_ver.ptr)):
            if a.select and a.select != sel_name:
                continue
            # the tracker: one update of the batch, first with room for every packet, then with room for its flows
            cap_flows = n
            for _ in range(2):
                lay = abi.flow_track_layout(cap_flows)
                d_state = ctx.alloc(lay["total"])
                ctx.flow_track_init(d_state, lay["total"], cap_flows)
                ctx.flow_track_update(d_state, run.batch, d_scratch, need, d_res, select=sel, batch_ts=7)
                ctx.synchronize()
                hdr = abi.FlowTrackHdr.from_bytes(d_state.download(np.zeros(128, np.uint8))).as_dict()
                nf = hdr["n_flows"]
                assert nf and not hdr["overflow_packets"]
                if nf == cap_flows:
                    break
                abi.Context.flow_track_forget(d_state)
                d_state.free()
                cap_flows = nf
            d_recs = d_state.ptr + lay["records"]
            tneed = abi.flow_track_top_scratch_bytes(cap_flows, max(KS))
            d_tscratch, d_tres = ctx.alloc(tneed), ctx.alloc(48)
            d_ids, d_vals, d_top = ctx.alloc(4 * max(KS)), ctx.alloc(8 * max(KS)), ctx.alloc(104 * max(KS))
            out = abi.FlowTopOut(d_ids.ptr, d_vals.ptr, d_top.ptr, None, d_tres.ptr)

            def top(metric, k, steps=a.steps):
                opts = abi.FlowTopOpts(metric, k, (ctypes.c_uint32 * 2)(0, 0))
                abi._check(L.bt_time_flow_top(ctx.h, d_state.ptr, ctypes.byref(opts), None, d_tscratch.ptr, tneed, ctypes.byref(out),
                                              steps, ms))
                return list(ms)[:steps]

            def result():
                return abi.FlowTopResult.from_bytes(d_tres.download(np.zeros(48, np.uint8))).as_dict()

            def timed(values, metric, k, check):
                top(metric, k)   # warm
                res = result()
                expect(res["status"] == 0 and res["n_flows"] == nf and res["n_top"] == min(k, nf) and res["metric"] == metric, f"{values} k={k}: result head")
                check(res, k)
                r = [med(top(metric, k)) for _ in range(a.rounds)]
                line(variant="flowtop", select=sel_name, values=values, metric=metric, k=k, flows=nf, flow_cap=cap_flows, n_ties=res["n_ties"],
                     threshold=res["threshold"], scratch_bytes=tneed, **stats(r), gflows=round(nf / (med(r) * 1e-3) / 1e9, 2))
                return res

            # what it replaces, and its own selection for the check
            host_top_total = {}
            cms, sms = (ctypes.c_float * a.host_steps)(), (ctypes.c_float * a.host_steps)()
            for k in KS:
                tot = ctypes.c_uint64(0)
                abi._check(L.bt_time_flow_top_host(ctx.h, d_recs, nf, k, a.host_steps, cms, sms, ctypes.byref(tot)))
                host_top_total[k] = tot.value
                both = [c + s for c, s in zip(cms, sms)]
                line(variant="host", select=sel_name, k=k, flows=nf, threads=1, d2h_ms=round(med(list(cms)), 4),
                     sort_ms=round(med(list(sms)), 4), **stats(both))

            def check_c3(res, k):
                expect(res["total"] == hdr["keyed_bytes"], "total differs from the header's keyed bytes")
                expect(res["top_total"] == host_top_total[k], "top_total differs from the host baseline's selection")

            for k in KS:
                timed("c3", abi.FLOW_TOP_BYTES, k, check_c3)

            moved = 104 * nf
            d_dst = ctx.alloc(moved + 256)

            def copy():
                abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_recs, moved, a.steps, ms))
                return med(list(ms))
            copy()
            r = stats([copy() for _ in range(a.rounds)])
            line(variant="copy", select=sel_name, bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)
            d_dst.free()

            # crafted records under the same header: random full-width byte counts, packets all zero
            rng = np.random.default_rng(nf)
            recs = np.zeros(nf, abi.FlowTrackRec)
            recs["bytes"][:, 0] = rng.integers(0, 1 << 64, nf, dtype=np.uint64)
            v = recs["bytes"][:, 0].copy()
            abi._check(L.bt_memcpy_h2d(ctx.h, d_recs, recs.ctypes.data, recs.nbytes))
            del recs
            want_total = int(v.sum(dtype=np.uint64))

            def check_random(res, k):
                kk = min(k, nf)
                expect(res["total"] == want_total, "total differs from numpy's")
                expect(res["threshold"] == int(np.partition(v, nf - kk)[nf - kk]), "the threshold differs from np.partition's")

            def check_equal(res, k):
                kk = min(k, nf)
                expect((res["threshold"], res["n_ties"], res["total"], res["top_total"]) == (0, nf, 0, 0), "the all-equal result")
                expect((d_ids.download(np.zeros(kk, np.uint32)) == np.arange(kk, dtype=np.uint32)).all(), "the all-equal top is not flows 0 .. k-1")

            for k in KS:
                timed("random", abi.FLOW_TOP_BYTES, k, check_random)
            for k in KS:
                timed("equal", abi.FLOW_TOP_PACKETS, k, check_equal)
            abi.Context.flow_track_forget(d_state)
            for b in (d_state, d_tscratch, d_tres, d_ids, d_vals, d_top):
                b.free()
        d_scratch.free()
        d_res.free()
        run.free()
    finally:
        ctx.close()
    if failed:
        line(variant="checks", failed=failed)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit(f"flowtop_rate: {len(failed)} checks failed")


if __name__ == "__main__":
    main()

"""The rate of the device-side flow table (bt_flow_table_device) and of what surrounds it.

  flowtab       the bench's C3 capture on the device, flow_id and flows written: the kernels
                (keys, insert, firsts, join, rank, emit) between an event pair recorded by the first
                and the last kernel's own dispatches; once with the `c3` program's verdict words as
                `select` (select=verdict) and once with select = NULL (select=all)
  fanout        bt_flow_fanout_device (8 queues, every output) on the same batch and selection
  filter_only   the filter-only bt_parse_filter_device (verdict + decide) on the same batch
                --baseline-lib PATH runs these two in a child process with that library (the parent
                commit's build) under BT_LIB_PATH; without it they come from this tree's library
  copy          one hipMemcpyAsync device-to-device of the bytes the call reads and writes: 64 B of
                header lines, the 8-B descriptor and select bit per packet in; per selected packet an
                80-B entry written and its 48-B key read, a 4-B owner word written and read per packet,
                the slots (4 B each) written once, 4 B of flow_id per packet and 80 B per flow out
  --flowtab-only runs the flowtab lines alone (a counter pass under rocprofv3 --pmc).
  host          what the call replaces: pass_idx copied to pinned host memory, then
                bt_flow_table_host over the listed frames on the calling thread, over the first
                --host-packets packets (their frames are downloaded for it); scaled_ms = that time
                scaled to the whole batch by packet count

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. The flow table's outputs are checked against bt_flow_table_host over the prefix
before they are timed.
Usage: python tools/flowtab_rate.py [--packets N] [--steps K] [--rounds R] [--baseline-lib PATH] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowtab/flowtab_rate.jsonl).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
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
    ap.add_argument("--host-packets", type=int, default=1 << 20)
    ap.add_argument("--baseline-lib", default=None, help="libbeatrice_gpu.so of the parent commit: fanout and filter_only from it")
    ap.add_argument("--baselines-only", action="store_true", help="the fanout and filter_only lines alone (the child)")
    ap.add_argument("--flowtab-only", action="store_true", help="the flowtab lines alone (for a counter pass)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowtab", "flowtab_rate.jsonl"))
    a = ap.parse_args()
    lines = []

    def line(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def rounds_of(fn):
        fn()   # warm
        r = [med(fn()) for _ in range(a.rounds)]
        return {"ms_median": round(med(r), 4), "ms_rounds": [round(x, 4) for x in sorted(r)]}

    lib_name = "baseline" if os.environ.get("BT_LIB_PATH") else "tree"
    ctx = abi.Context(0)
    L = abi.lib()
    try:
        wl = bench.WORKLOADS["c3"]
        cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
        run, n = cap.run, cap.n
        tiles = (n + 63) // 64
        ctx.compile(wl["filters"])
        ctx.reserve(n)
        ctx.run_device(run.batch, run.outs)   # verdict, decide, pass_idx, n_pass
        ctx.synchronize()
        n_pass = int(run.d_npass.download(np.zeros(1, np.uint32))[0])
        ms, ms2 = (ctypes.c_float * a.steps)(), (ctypes.c_float * a.steps)()

        if a.baselines_only or not (a.baseline_lib or a.flowtab_only):
            K = 8
            fopts = abi.FanoutOpts.make(K)
            bufs = [ctx.alloc(4 * n), ctx.alloc(n), ctx.alloc(4 * n), ctx.alloc(8 * K * tiles), ctx.alloc(ctypes.sizeof(abi.FanoutResult))]
            fout = abi.FanoutOut(*[b.ptr for b in bufs])
            for sel_name, sel in (("verdict", run.d_ver.ptr), ("all", None)):
                def fanout():
                    abi._check(L.bt_time_fanout(ctx.h, ctypes.byref(run.batch), sel, ctypes.byref(fopts), ctypes.byref(fout),
                                                a.steps, ms))
                    return list(ms)
                line(variant="fanout", lib=lib_name, select=sel_name, packets=n, queues=K, **rounds_of(fanout))
            for b in bufs:
                b.free()
            fo = abi.Outputs(None, 0, run.d_ver.ptr, run.d_dec.ptr, None, None)
            line(variant="filter_only", lib=lib_name, packets=n, **rounds_of(lambda: [ctx.time_device(run.batch, fo, a.steps)[0]]))
        if not a.baselines_only:
            need = abi.flow_table_scratch_bytes(n, 0)
            slots = 128
            while slots < 2 * n:
                slots *= 2
            d_scratch, d_id, d_flows = ctx.alloc(need), ctx.alloc(4 * n), ctx.alloc(80 * n)
            d_res = ctx.alloc(ctypes.sizeof(abi.FlowTableResult))
            opts = abi.FlowTableOpts(0, 0, n, 0)
            out = abi.FlowTableOut(d_id.ptr, d_flows.ptr, d_res.ptr)
            m = min(n, a.host_packets)
            desc = cap.desc[:m]
            end = int(synth.desc_off(desc)[-1] + synth.desc_len(desc)[-1])
            frames = run.d_data.download(np.zeros(end, np.uint8))
            ver = run.d_ver.download(np.zeros(tiles, np.uint64))
            for sel_name, sel in (("verdict", run.d_ver.ptr), ("all", None)):
                def flowtab():
                    abi._check(L.bt_time_flow_table(ctx.h, ctypes.byref(run.batch), sel, ctypes.byref(opts), d_scratch.ptr, need,
                                                    ctypes.byref(out), a.steps, ms))
                    return list(ms)
                flowtab()
                res = abi.FlowTableResult.from_bytes(d_res.download(np.zeros(d_res.nbytes, np.uint8))).as_dict()
                # the outputs are right before they are timed: a prefix against the host table (flows are
                # numbered by first packet, so the prefix's ids and first packets are the host's over the prefix)
                hid, hflows, hres = abi.flow_table_host(frames, desc, abi.FlowTableOpts(0, 0, m, 0),
                                                        None if sel is None else ver[:(m + 63) // 64])
                got_id = d_id.download(np.zeros(m, np.uint32))
                assert (got_id == hid).all(), "flow_id differs from the host table over the prefix"
                got = d_flows.download(np.zeros(80 * hres["n_flows"], np.uint8)).view(abi.FlowRec)
                assert (got["first"] == hflows["first"]).all() and (got["key"] == hflows["key"]).all()
                assert res["n"] == n and res["overflow_packets"] == 0 and res["n_selected"] == (n if sel is None else n_pass)
                line(variant="flowtab", select=sel_name, packets=n, selected=res["n_selected"], flows=res["n_flows"],
                     slots=res["slots"], scratch_bytes=need, **rounds_of(flowtab),
                     gpps=round(n / (med(flowtab()) * 1e-3) / 1e9, 2))
                if a.flowtab_only:
                    continue
                ns = res["n_selected"]
                moved = n * (64 + 8) + tiles * 8 + (80 + 48) * ns + 2 * 4 * n + 4 * slots + 4 * n + 80 * res["n_flows"]
                d_src, d_dst = ctx.alloc(moved + 256), ctx.alloc(moved + 256)

                def copy():
                    abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_src.ptr, moved, a.steps, ms))
                    return list(ms)
                r = rounds_of(copy)
                line(variant="copy", select=sel_name, bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)
                d_src.free()
                d_dst.free()
            # host: the pass list's prefix that lies in the downloaded frames
            pidx = run.d_pidx.download(np.zeros(n_pass, np.uint32))
            mp = 0 if a.flowtab_only else int(np.searchsorted(pidx, m))
            hopts = abi.FlowTableOpts(0, 0, 0, 0)
            last = abi.FlowTableResult()

            def host():
                abi._check(L.bt_time_flow_table_host(ctx.h, run.d_pidx.ptr, mp, frames.ctypes.data, len(frames), desc.ctypes.data,
                                                     ctypes.byref(hopts), a.steps, ms, ms2, ctypes.byref(last)))
                return list(ms), list(ms2)

            rounds = [host() for _ in range(a.rounds + 1)][1:] if mp else []
            cp, tb = (med([med(c) for c, _ in rounds]), med([med(b) for _, b in rounds])) if mp else (0.0, 0.0)
            if mp:
                line(variant="host", packets=m, listed=mp, flows=int(last.n_flows), threads=1, d2h_ms=round(cp, 4), table_ms=round(tb, 4),
                     ms_median=round(cp + tb, 4), scaled_ms=round((cp + tb) * n_pass / max(mp, 1), 3))
            for b in (d_scratch, d_id, d_flows, d_res):
                b.free()
        run.free()
    finally:
        ctx.close()
    if a.baseline_lib and not a.baselines_only and not a.flowtab_only:   # the parent's library, in a process of its own
        env = dict(os.environ, BT_LIB_PATH=os.path.abspath(a.baseline_lib),
                   LD_LIBRARY_PATH=os.path.dirname(os.path.abspath(a.baseline_lib)) + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baselines-only", "--packets", str(a.packets), "--steps",
                            str(a.steps), "--rounds", str(a.rounds), "--out", ""], env=env, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f"flowtab_rate: the child failed: {r.stderr[-2000:]}")
        for ln in r.stdout.strip().splitlines():
            if ln.startswith("{"):
                lines.append(ln)
                print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

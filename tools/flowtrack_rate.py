"""The rate of the flow tracker's update (bt_flow_track_update_device) and of what surrounds it, on
the bench's C3 capture on the device, once with the `c3` program's verdict words as `select`
(select=verdict) and once with select = NULL (select=all), flow_id written.

  flowtrack     an update call: the per-batch table's kernels and find, join, apply, ids between an
                event pair recorded by the first and the last kernel's own dispatches, on two streams:
                stream=repeat  the batch merged into a state that already holds its flows (every flow
                               is found: flows that repeat across batches)
                stream=new     the batch merged into an empty state (every flow is new); the state is
                               initialised again before each timed call
  flowtab       bt_flow_table_device with flow_cap = n on the same batch and selection: the update
                minus this is the cost of the merge passes alone. --baseline-lib PATH runs it in a
                child process with that library (the parent commit's build) under BT_LIB_PATH;
                without it, it comes from this tree's library
  copy          one hipMemcpyAsync device-to-device of the bytes the merge reads and writes per flow
                of the batch: its 80-B record read twice (find, apply), a 4-B map entry written and
                read, a slot word and a 40-B key read, a 104-B record read and written (repeat) or
                written with a slot word (new); and 4 B of flow_id read and written per packet
  host          what the update replaces (tools/pcap_flows.py's per-chunk path): the batch's flow
                records copied to pinned host memory, then merged into a host tracker state on the
                calling thread (repeat: the state holds them; new: the state is empty each time)

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the state after two updates is checked against
bt_flow_track_update_host over a prefix of the batch.
Usage: python tools/flowtrack_rate.py [--packets N] [--steps K] [--rounds R] [--baseline-lib PATH] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowtrack/flowtrack_rate.jsonl).
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
    ap.add_argument("--check-packets", type=int, default=1 << 18)
    ap.add_argument("--baseline-lib", default=None, help="libbeatrice_gpu.so of the parent commit: the flowtab lines from it")
    ap.add_argument("--baselines-only", action="store_true", help="the flowtab lines alone (the child)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowtrack", "flowtrack_rate.jsonl"))
    a = ap.parse_args()
    lines = []

    def line(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def stats(r):
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
        ctx.run_device(run.batch, run.outs)   # verdict words
        ctx.synchronize()
        ms, ms2 = (ctypes.c_float * a.steps)(), (ctypes.c_float * a.steps)()
        d_id, d_flows = ctx.alloc(4 * n), ctx.alloc(80 * n)
        d_tres = ctx.alloc(ctypes.sizeof(abi.FlowTableResult))
        selections = (("verdict", run.d_ver.ptr), ("all", None))

        if a.baselines_only or not a.baseline_lib:
            need = abi.flow_table_scratch_bytes(n, 0)
            d_scratch = ctx.alloc(need)
            opts = abi.FlowTableOpts(0, 0, n, 0)
            out = abi.FlowTableOut(d_id.ptr, d_flows.ptr, d_tres.ptr)
            for sel_name, sel in selections:
                def flowtab():
                    abi._check(L.bt_time_flow_table(ctx.h, ctypes.byref(run.batch), sel, ctypes.byref(opts), d_scratch.ptr, need,
                                                    ctypes.byref(out), a.steps, ms))
                    return med(list(ms))
                flowtab()
                res = abi.FlowTableResult.from_bytes(d_tres.download(np.zeros(d_tres.nbytes, np.uint8))).as_dict()
                line(variant="flowtab", lib=lib_name, select=sel_name, packets=n, flows=res["n_flows"],
                     **stats([flowtab() for _ in range(a.rounds)]))
            d_scratch.free()
        if not a.baselines_only:
            need = abi.flow_track_scratch_bytes(n)
            d_scratch, d_res = ctx.alloc(need), ctx.alloc(64)
            upd, out = abi.FlowTrackUpdate(None, 7), abi.FlowTrackOut(d_id.ptr, d_res.ptr)
            topts = abi.FlowTableOpts(0, 0, n, 0)
            tneed = abi.flow_table_scratch_bytes(n, 0)
            for sel_name, sel in selections:
                # the batch's flows, for the capacity and for the host baseline
                ctx.flow_table_device(run.batch, topts, d_scratch, tneed, d_tres, select=sel, flows=d_flows)
                ctx.synchronize()
                nf = abi.FlowTableResult.from_bytes(d_tres.download(np.zeros(d_tres.nbytes, np.uint8))).as_dict()["n_flows"]
                cap_flows = max(nf, 1)
                lay = abi.flow_track_layout(cap_flows)
                d_state = ctx.alloc(lay["total"])

                def update(steps):
                    abi._check(L.bt_time_flow_track(ctx.h, d_state.ptr, ctypes.byref(run.batch), sel, ctypes.byref(upd), d_scratch.ptr,
                                                    need, ctypes.byref(out), steps, ms))
                    return list(ms)[:steps]

                def result():
                    return abi.FlowTrackResult.from_bytes(d_res.download(np.zeros(64, np.uint8))).as_dict()

                # right before it is timed: two updates of a prefix against the host form, header and records
                m = min(n, a.check_packets)
                desc = cap.desc[:m]
                end = int(synth.desc_off(desc)[-1] + synth.desc_len(desc)[-1])
                frames = run.d_data.download(np.zeros(end, np.uint8))
                ver = None if sel is None else run.d_ver.download(np.zeros(tiles, np.uint64))[:(m + 63) // 64]
                host = abi.HostFlowTracker(cap_flows)
                ctx.flow_track_init(d_state, lay["total"], cap_flows)
                pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, run.batch.bytes, run.batch.desc_format, 0)
                for _ in range(2):
                    ctx.flow_track_update(d_state, pre, d_scratch, need, d_res, select=sel, batch_ts=7, flow_id=d_id)
                    hid, hres = host.update(frames, desc, ver, None, 7)
                ctx.synchronize()
                assert result() == hres and (d_id.download(np.zeros(m, np.uint32)) == hid).all(), "the update differs from the host form"
                both = d_state.download(np.zeros(lay["records"] + 104 * hres["n_flows"], np.uint8))
                assert both[:128].tobytes() == host.state[:128].tobytes() and \
                    both[lay["records"]:].tobytes() == host.state[lay["records"]:lay["records"] + 104 * hres["n_flows"]].tobytes()

                # repeat: the state holds the batch's flows
                ctx.flow_track_init(d_state, lay["total"], cap_flows)
                update(1)
                assert result()["new_flows"] == nf
                update(a.steps)   # warm
                r = [med(update(a.steps)) for _ in range(a.rounds)]
                res = result()
                assert res["new_flows"] == 0 and res["overflow_flows"] == 0 and res["batch_flows"] == nf and res["status"] == 0
                line(variant="flowtrack", stream="repeat", select=sel_name, packets=n, selected=res["n_selected"], flows=nf,
                     slots=lay["slots"], scratch_bytes=need, state_bytes=lay["total"], **stats(r),
                     gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
                # new: an empty state before every timed call
                r = []
                for k in range(a.rounds * 2 + 1):
                    ctx.flow_track_init(d_state, lay["total"], cap_flows)
                    t = update(1)[0]
                    if k:
                        r.append(t)
                res = result()
                assert res["new_flows"] == nf and res["overflow_flows"] == 0
                line(variant="flowtrack", stream="new", select=sel_name, packets=n, selected=res["n_selected"], flows=nf,
                     slots=lay["slots"], **stats(r), gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
                # copy: the bytes of the merge passes
                for stream, per_flow in (("repeat", 2 * 80 + 2 * 4 + 4 + 40 + 2 * 104), ("new", 2 * 80 + 2 * 4 + 4 + 104 + 4)):
                    moved = nf * per_flow + 2 * 4 * n
                    d_src, d_dst = ctx.alloc(moved + 256), ctx.alloc(moved + 256)

                    def copy():
                        abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_src.ptr, moved, a.steps, ms))
                        return med(list(ms))
                    copy()
                    r = stats([copy() for _ in range(a.rounds)])
                    line(variant="copy", stream=stream, select=sel_name, bytes=moved, gbps=round(moved / (r["ms_median"] * 1e-3) / 1e9, 1), **r)
                    d_src.free()
                    d_dst.free()
                # host: the flows' records over PCIe, then the merge on one thread
                if nf:
                    last = abi.FlowTrackResult()
                    for stream in ("repeat", "new"):
                        cps, mgs = [], []
                        for k in range(a.rounds + 1):
                            host = abi.HostFlowTracker(cap_flows)
                            steps = a.steps if stream == "repeat" else 1
                            if stream == "repeat":   # the state holds the flows before the timed merges
                                abi._check(L.bt_time_flow_track_host(ctx.h, d_flows.ptr, nf, host.state.ctypes.data, host.state.nbytes, 7, 1,
                                                                     ms, ms2, ctypes.byref(last)))
                            abi._check(L.bt_time_flow_track_host(ctx.h, d_flows.ptr, nf, host.state.ctypes.data, host.state.nbytes, 7, steps,
                                                                 ms, ms2, ctypes.byref(last)))
                            if k:
                                cps.append(med(list(ms)[:steps]))
                                mgs.append(med(list(ms2)[:steps]))
                            assert last.new_flows == (0 if stream == "repeat" else nf) and last.overflow_flows == 0
                        line(variant="host", stream=stream, select=sel_name, flows=nf, threads=1, d2h_ms=round(med(cps), 4),
                             merge_ms=round(med(mgs), 4), ms_median=round(med(cps) + med(mgs), 4))
                abi.Context.flow_track_forget(d_state)
                d_state.free()
            for b in (d_scratch, d_res):
                b.free()
        for b in (d_id, d_flows, d_tres):
            b.free()
        run.free()
    finally:
        ctx.close()
    if a.baseline_lib and not a.baselines_only:   # the parent's library, in a process of its own
        env = dict(os.environ, BT_LIB_PATH=os.path.abspath(a.baseline_lib),
                   LD_LIBRARY_PATH=os.path.dirname(os.path.abspath(a.baseline_lib)) + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baselines-only", "--packets", str(a.packets), "--steps",
                            str(a.steps), "--rounds", str(a.rounds), "--out", ""], env=env, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f"flowtrack_rate: the child failed: {r.stderr[-2000:]}")
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

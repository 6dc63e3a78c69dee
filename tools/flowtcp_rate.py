"""The rate of the TCP side table's update (bt_flow_tcp_update_device) and of what surrounds it, on
the bench's C3 capture on the device, every packet selected.

  flowtcp       the update's kernel between an event pair recorded by its own dispatch, on three id streams:
                ids=tracker   the flow numbers bt_flow_track_update_device gave the batch
                ids=one       every packet numbered 0: a batch that is one flow (flow_cap = 1)
                ids=distinct  packet i numbered i: every packet its own flow (flow_cap = n)
                The table is zero before the first call; the timed calls find every flag bit set
                (no atomicOr) and still add the SYN / FIN / RST counts.
  flowtrack     the tracker's update of the same batch into a state that holds its flows, flow_id
                written: bt_flowtab_keys is its first kernel (its own time comes from a kernel trace of
                this variant). --baseline-lib PATH runs it in a child process with that library (the
                parent commit's build) under BT_LIB_PATH; without it, it comes from this tree's library
  copy          one hipMemcpyAsync device-to-device of the batch's frame bytes

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before anything is timed the side table of a prefix of the batch is checked
against bt_flow_tcp_update_host.
Usage: python tools/flowtcp_rate.py [--packets N] [--steps K] [--rounds R] [--baseline-lib PATH] [--only VARIANT] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowtcp/flowtcp_rate.jsonl).
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
    ap.add_argument("--baseline-lib", default=None, help="libbeatrice_gpu.so of the parent commit: the flowtrack line from it")
    ap.add_argument("--baselines-only", action="store_true", help="the flowtrack line alone (the child, or a kernel trace)")
    ap.add_argument("--only", default=None, help="one flowtcp id stream alone (a counter run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowtcp", "flowtcp_rate.jsonl"))
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
        ctx.reserve(n)
        ms = (ctypes.c_float * a.steps)()
        d_id = ctx.alloc(4 * n)
        need = abi.flow_track_scratch_bytes(n)
        d_scratch, d_res = ctx.alloc(need), ctx.alloc(64)
        lay = abi.flow_track_layout(n)
        d_state = ctx.alloc(lay["total"])
        ctx.flow_track_init(d_state, lay["total"], n)
        upd, out = abi.FlowTrackUpdate(None, 7), abi.FlowTrackOut(d_id.ptr, d_res.ptr)

        def track(steps):
            abi._check(L.bt_time_flow_track(ctx.h, d_state.ptr, ctypes.byref(run.batch), None, ctypes.byref(upd), d_scratch.ptr, need,
                                            ctypes.byref(out), steps, ms))
            return list(ms)[:steps]

        track(1)   # the state holds the batch's flows, d_id their numbers
        res = abi.FlowTrackResult.from_bytes(d_res.download(np.zeros(64, np.uint8))).as_dict()
        nf = res["n_flows"]
        assert res["overflow_flows"] == 0 and res["status"] == 0
        if a.baselines_only or not a.baseline_lib:
            track(a.steps)   # warm
            r = [med(track(a.steps)) for _ in range(a.rounds)]
            line(variant="flowtrack", lib=lib_name, stream="repeat", select="all", packets=n, flows=nf, **stats(r),
                 gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
        if not a.baselines_only:
            d_tres = ctx.alloc(32)
            # right before it is timed: a prefix against the host form, table and result
            m = min(n, a.check_packets)
            desc = cap.desc[:m]
            end = int(synth.desc_off(desc)[-1] + synth.desc_len(desc)[-1])
            frames = run.d_data.download(np.zeros(end, np.uint8))
            ids = d_id.download(np.zeros(m, np.uint32))
            d_tcp = ctx.alloc(16 * n)
            d_tcp.zero()
            pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, run.batch.bytes, run.batch.desc_format, 0)
            ctx.flow_tcp_update(pre, d_id, 0, d_tcp, n, d_tres)
            ctx.synchronize()
            host = np.zeros(n, abi.FlowTcpRec)
            hres = abi.flow_tcp_update_host(frames, desc, ids, 0, host)
            assert abi.FlowTcpResult.from_bytes(d_tres.download(np.zeros(32, np.uint8))).as_dict() == hres, "the update differs from the host form"
            assert d_tcp.download(np.zeros(16 * n, np.uint8)).tobytes() == host.tobytes(), "the side table differs from the host form"
            d_tcp.free()

            streams = (("tracker", None, n), ("one", np.zeros(n, np.uint32), 1), ("distinct", np.arange(n, dtype=np.uint32), n))
            for name, ids, flow_cap in streams:
                if a.only and a.only != name:
                    continue
                d_ids = d_id
                if ids is not None:
                    d_ids = ctx.alloc(4 * n)
                    d_ids.upload(ids)
                d_tcp = ctx.alloc(16 * flow_cap)
                d_tcp.zero()

                def update():
                    abi._check(L.bt_time_flow_tcp(ctx.h, ctypes.byref(run.batch), d_ids.ptr, 0, d_tcp.ptr, flow_cap, d_tres.ptr, a.steps, ms))
                    return list(ms)
                first = update()   # the first call of it sets the bits
                r = [med(update()) for _ in range(a.rounds)]
                t = abi.FlowTcpResult.from_bytes(d_tres.download(np.zeros(32, np.uint8))).as_dict()
                assert t["n"] == n and t["bad_ids"] == 0 and t["tcp_packets"] > 0
                line(variant="flowtcp", ids=name, packets=n, flow_cap=flow_cap, tcp_packets=t["tcp_packets"], syn=t["syn_packets"],
                     fin=t["fin_packets"], rst=t["rst_packets"], first_call_ms=round(first[0], 4), **stats(r),
                     gpps=round(n / (med(r) * 1e-3) / 1e9, 2))
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
            d_tres.free()
        abi.Context.flow_track_forget(d_state)
        for b in (d_id, d_scratch, d_res, d_state):
            b.free()
        run.free()
    finally:
        ctx.close()
    if a.baseline_lib and not a.baselines_only and not a.only:   # the parent's library, in a process of its own
        env = dict(os.environ, BT_LIB_PATH=os.path.abspath(a.baseline_lib),
                   LD_LIBRARY_PATH=os.path.dirname(os.path.abspath(a.baseline_lib)) + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--baselines-only", "--packets", str(a.packets), "--steps",
                            str(a.steps), "--rounds", str(a.rounds), "--out", ""], env=env, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f"flowtcp_rate: the child failed: {r.stderr[-2000:]}")
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

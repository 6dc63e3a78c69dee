"""The rate of the device-side fan-out (bt_flow_fanout_device) and of what surrounds it.

  fanout        the bench's C3 capture on the device, K queues, the `c3` program's verdict words as
                `select`, every output: the three kernels between an event pair recorded by the
                first and the last kernel's own dispatches, for the Toeplitz form of this process
                (BT_FANOUT_TABLE: 1 = nibble tables in LDS, the default; 0 = bit-serial, key in SGPRs)
  fanout_other  the same in a child process with the knob the other way
  filter_only   the filter-only bt_parse_filter_device (verdict + decide) on the same batch
  host          what the call replaces: pass_idx copied to pinned host memory, then the host key,
                hash and stable bucket in 16 parts on the context's host threads, over the first
                --host-packets packets (their frames are downloaded for it); scaled_ms = that
                time scaled to the whole batch by packet count
  copy          one hipMemcpyAsync device-to-device of the bytes the call reads and writes: 64 B
                of header lines, the 8-B descriptor and select bit per packet in; 4 + 1 + K / 8 B
                per packet and 4 B per selected packet out: the floor

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. The fan-out's outputs are checked against the host hash before they are timed.
Usage: python tools/fanout_rate.py [--packets N] [--queues K] [--steps K] [--rounds R] [--out FILE]
Prints one JSON line per variant (also appended to --out).
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
    ap.add_argument("--queues", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-packets", type=int, default=1 << 20)
    ap.add_argument("--fanout-only", action="store_true", help="the fanout line alone (the child of the A/B)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    form = "table" if os.environ.get("BT_FANOUT_TABLE", "1") != "0" else "serial"
    lines = []

    def line(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    ctx = abi.Context(0)
    L = abi.lib()
    try:
        wl = bench.WORKLOADS["c3"]
        cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
        run, n, K = cap.run, cap.n, a.queues
        tiles = (n + 63) // 64
        ctx.compile(wl["filters"])
        ctx.reserve(n)
        ctx.run_device(run.batch, run.outs)   # verdict, decide, pass_idx, n_pass
        ctx.synchronize()
        n_pass = int(run.d_npass.download(np.zeros(1, np.uint32))[0])
        opts = abi.FanoutOpts.make(K)
        d_hash, d_queue, d_idx = ctx.alloc(4 * n), ctx.alloc(n), ctx.alloc(4 * n)
        d_rows, d_res = ctx.alloc(8 * K * tiles), ctx.alloc(ctypes.sizeof(abi.FanoutResult))
        out = abi.FanoutOut(d_hash.ptr, d_queue.ptr, d_idx.ptr, d_rows.ptr, d_res.ptr)
        ms, ms2 = (ctypes.c_float * a.steps)(), (ctypes.c_float * a.steps)()

        def fanout():
            abi._check(L.bt_time_fanout(ctx.h, ctypes.byref(run.batch), run.d_ver.ptr, ctypes.byref(opts),
                                        ctypes.byref(out), a.steps, ms))
            return list(ms)

        fanout()   # warm: code objects, the workspace, first touch of the buffers
        # the outputs are right before they are timed: the first packets against the host hash
        m = min(n, a.host_packets)
        desc = cap.desc[:m]
        end = int(synth.desc_off(desc)[-1] + synth.desc_len(desc)[-1])
        frames = run.d_data.download(np.zeros(end, np.uint8))
        res = abi.FanoutResult.from_bytes(d_res.download(np.zeros(d_res.nbytes, np.uint8))).as_dict()
        got_h, got_q = d_hash.download(np.zeros(m, np.uint32)), d_queue.download(np.zeros(m, np.uint8))
        ver = np.unpackbits(run.d_ver.download(np.zeros(tiles, np.uint64)).view(np.uint8), bitorder="little")[:n]
        offs, lens = synth.desc_off(desc).astype(np.int64), synth.desc_len(desc).astype(np.int64)
        for i in range(0, m, max(1, m // 4096)):
            h, _, q = abi.flow_hash_host(frames[offs[i]:offs[i] + lens[i]], opts)
            assert got_h[i] == h and got_q[i] == (q if ver[i] else 0xFF), f"packet {i}: device differs from the host hash"
        assert res["n"] == n and res["n_selected"] == n_pass == int(ver.sum()) and res["start"][K] == n_pass
        res_fan = [med(fanout()) for _ in range(a.rounds)]
        per_q = [res["start"][q + 1] - res["start"][q] for q in range(K)]
        line(variant="fanout", form=form, packets=n, queues=K, selected=n_pass, per_queue=per_q,
             ms_median=round(med(res_fan), 4), ms_rounds=[round(x, 4) for x in sorted(res_fan)],
             gpps=round(n / (med(res_fan) * 1e-3) / 1e9, 2))
        if not a.fanout_only:
            fo = abi.Outputs(None, 0, run.d_ver.ptr, run.d_dec.ptr, None, None)
            ctx.time_device(run.batch, fo, a.steps)
            res_f = [ctx.time_device(run.batch, fo, a.steps)[0] for _ in range(a.rounds)]
            line(variant="filter_only", packets=n, ms_median=round(med(res_f), 4), ms_rounds=[round(x, 4) for x in sorted(res_f)])
            # host: the pass list's prefix that lies in the downloaded frames
            pidx = run.d_pidx.download(np.zeros(n_pass, np.uint32))
            mp = int(np.searchsorted(pidx, m))
            counts = (ctypes.c_uint32 * 65)()

            def host():
                abi._check(L.bt_time_fanout_host(ctx.h, run.d_pidx.ptr, mp, frames.ctypes.data, desc.ctypes.data,
                                                 ctypes.byref(opts), a.steps, ms, ms2, counts))
                return list(ms), list(ms2)

            host()
            rounds = [host() for _ in range(a.rounds)]
            cp, bk = med([med(c) for c, _ in rounds]), med([med(b) for _, b in rounds])
            line(variant="host", packets=m, listed=mp, threads=min(16, abi.usable_cpus()), d2h_ms=round(cp, 4),
                 bucket_ms=round(bk, 4), ms_median=round(cp + bk, 4), scaled_ms=round((cp + bk) * n_pass / max(mp, 1), 3))
            moved = n * (64 + 8) + tiles * 8 + n * 5 + K * tiles * 8 + 4 * n_pass
            d_src, d_dst = ctx.alloc(moved + 256), ctx.alloc(moved + 256)

            def copy():
                abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_src.ptr, moved, a.steps, ms))
                return list(ms)

            copy()
            res_c = [med(copy()) for _ in range(a.rounds)]
            line(variant="copy", bytes=moved, ms_median=round(med(res_c), 4), ms_rounds=[round(x, 4) for x in sorted(res_c)],
                 gbps=round(moved / (med(res_c) * 1e-3) / 1e9, 1))
            d_src.free()
            d_dst.free()
        for b in (d_hash, d_queue, d_idx, d_rows, d_res):
            b.free()
        run.free()
    finally:
        ctx.close()
    if not a.fanout_only:   # the other Toeplitz form, in a process of its own: the knob is read once
        env = dict(os.environ, BT_FANOUT_TABLE="0" if form == "table" else "1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fanout-only", "--packets", str(a.packets),
                            "--queues", str(a.queues), "--steps", str(a.steps), "--rounds", str(a.rounds),
                            "--host-packets", str(a.host_packets)], env=env, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f"fanout_rate: the child failed: {r.stderr[-2000:]}")
        other = json.loads(r.stdout.strip().splitlines()[-1])
        other["variant"] = "fanout_other"
        lines.append(json.dumps(other))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""The rate of the device-side counts (bt_tally_device) and of what they replace.

  tally_decide  the bench's C3 capture on the device, the `c3` program's decision bytes: both tally
                kernels between an event pair from their own dispatches, decisions only
  tally_full    ... decisions + frame lengths + records (byte sums and layer counts too)
  copy_decide   one hipMemcpyAsync device-to-device of the decision bytes (n B) ...
  copy_full     ... and of as many bytes as tally_full reads: decisions (1 B), 8-B descriptors and
                the records' slab-1 regions (16 B, the dword sits at a 16-B stride) per packet,
                in the same process, alternating round by round: the ceiling for those bytes
  host          what the tally replaces: the decision bytes copied to pinned host memory plus the
                16-part host scan of scanParallel's inner loop on the context's host threads

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. BT_TALLY_PEEL=0 in the environment selects the histogram by LDS adds instead
of ballot peeling.
Usage: python tools/tally_rate.py [--packets N] [--steps K] [--rounds R]
Prints one JSON line per variant and a last line with the ratios.
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


def line(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ctx = abi.Context(0)
    L = abi.lib()
    try:
        wl = bench.WORKLOADS["c3"]
        cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
        run, n = cap.run, cap.n
        ctx.compile(wl["filters"])
        ctx.run_device(run.batch, abi.Outputs(run.outs.records, n, None, run.outs.decide, None, None))
        ctx.synchronize()
        dec = run.d_dec.download(np.zeros(n, np.uint8))
        lens = synth.desc_len(cap.desc).astype(np.int64)
        full_bytes = n * (1 + 8 + 16)
        d_tally = ctx.alloc(ctypes.sizeof(abi.Tally))
        d_src, d_dst = ctx.alloc(full_bytes + 256), ctx.alloc(full_bytes + 256)
        ms, ms2 = (ctypes.c_float * a.steps)(), (ctypes.c_float * a.steps)()
        counts = (ctypes.c_uint64 * 2)()

        def tally(frames, records):
            abi._check(L.bt_time_tally(ctx.h, run.d_dec.ptr, n, ctypes.byref(run.batch) if frames else None,
                                       run.d_rec.ptr if records else None, n, 0, d_tally.ptr, a.steps, ms))
            return list(ms)

        def copy(nbytes):
            abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_src.ptr, nbytes, a.steps, ms))
            return list(ms)

        def host():
            abi._check(L.bt_time_tally_host(ctx.h, run.d_dec.ptr, n, a.steps, ms, ms2, counts))
            return [x + y for x, y in zip(ms, ms2)], list(ms), list(ms2)

        variants = {"tally_decide": lambda: tally(False, False), "tally_full": lambda: tally(True, True),
                    "copy_decide": lambda: copy(n), "copy_full": lambda: copy(full_bytes), "host": lambda: host()[0]}
        for fn in variants.values():   # warm: code objects, the workspace, first touch of the buffers
            fn()
        # the counts are right before they are timed
        t = abi.Tally.from_bytes(d_tally.download(np.zeros(d_tally.nbytes, np.uint8))).as_dict()
        hist = np.bincount(dec, minlength=256).reshape(4, 64)
        assert t["slot"] == hist.tolist() and t["n"] == n, "tally differs from numpy over the decision bytes"
        assert t["bytes"] == [int(lens[dec >> 6 == k].sum()) for k in range(4)]
        thrown = np.nonzero(dec >> 6 >= 2)[0]
        upto = int(thrown[0]) if len(thrown) else n
        assert (counts[0], counts[1]) == (upto, int((dec[:upto] >> 6 == 0).sum())), "host scan differs"
        res = {v: [] for v in variants}
        parts = {"copy": [], "scan": []}
        for _ in range(a.rounds):
            for v in variants:
                if v == "host":
                    tot, c, s = host()
                    res[v].append(med(tot))
                    parts["copy"].append(med(c))
                    parts["scan"].append(med(s))
                else:
                    res[v].append(med(variants[v]()))
        m = {v: med(x) for v, x in res.items()}
        read = {"tally_decide": n, "tally_full": full_bytes, "copy_decide": n, "copy_full": full_bytes, "host": n}
        for v in variants:
            extra = {"d2h_ms": round(med(parts["copy"]), 4), "scan_ms": round(med(parts["scan"]), 4),
                     "threads": min(16, abi.usable_cpus())} if v == "host" else {}
            line(variant=v, packets=n, in_bytes=read[v], ms_median=round(m[v], 4),
                 ms_rounds=[round(x, 4) for x in sorted(res[v])], in_gbps=round(read[v] / (m[v] * 1e-3) / 1e9, 1),
                 gpps=round(n / (m[v] * 1e-3) / 1e9, 2), **extra)
        line(summary={"peel": os.environ.get("BT_TALLY_PEEL", "1"),
                      "tally_decide_over_host": round(m["tally_decide"] / m["host"], 4),
                      "tally_decide_over_copy_decide": round(m["tally_decide"] / m["copy_decide"], 3),
                      "tally_full_over_copy_full": round(m["tally_full"] / m["copy_full"], 3)})
        for b in (d_tally, d_src, d_dst):
            b.free()
        run.free()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()

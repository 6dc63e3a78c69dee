"""What the two-pass PAYLOAD form costs: one C3 capture on the device at the bench's size, filter
only, timed with HIP events on a caller stream (a warm-up first), alternating the variants round
by round in one process, for two programs:

  first   /GET|POST/ + C3's chain    the PAYLOAD slot first: every frame is a work item
  last    C3's udp + 10.0.0.0/8, then /GET|POST/   few frames reach the slot

  fused        bt_parse_filter_device over the whole frames (the single-pass kernel)
  prefix       the same batch with BT_BATCH_PREFIXES (the first pass alone: HOST at the slot)
  two_pass     prefix + bt_filter_resume_device over the whole frames (decide rewritten in place)
  resume       two_pass - prefix, the second pass's own cost (the resume kernel, the verdict
               rebuild and the compaction)

and the TPACKET_V3 ring stage over a registered ring of --ring-packets C3 frames (wall clock per
call, the host walk included): in place, lean gather without the second pass (its PAYLOAD frames
stay HOST) and lean gather + BT_RING_RESUME_PAYLOAD, each checked against the in-place decisions.

Usage: python tools/payload_resume_rate.py [--packets N] [--steps K] [--rounds R] [--ring-packets M]
Prints one JSON line per program and variant.
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

EXPR = "GET|POST"
PROGRAMS = {"first": [{"type": abi.PAYLOAD, "expr": EXPR, "priority": 9}] + bench.C3_FILTERS,
            "last": bench.C3_FILTERS[:2] + [{"type": abi.PAYLOAD, "expr": EXPR, "priority": 0}]}


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


class HipEvents:
    """hipEvent_t pairs through the HIP runtime the library itself is linked against."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.e0, self.e1):
            self.ok(self.hip.hipEventCreate(ctypes.byref(e)))

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError(f"HIP error {rc}")

    def start(self, stream):
        self.ok(self.hip.hipEventRecord(self.e0, stream))

    def stop_ms(self, stream) -> float:
        self.ok(self.hip.hipEventRecord(self.e1, stream))
        self.ok(self.hip.hipEventSynchronize(self.e1))
        ms = ctypes.c_float()
        self.ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.e0, self.e1))
        return ms.value


def device_part(ctx, a):
    wl = dict(bench.WORKLOADS["c3"], payload=EXPR)
    cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets)
    run = cap.run
    n = run.n
    outs = abi.Outputs(None, n, run.outs.verdict, run.outs.decide, run.outs.pass_idx, run.outs.n_pass)
    s = ctx.stream_create()
    ev = HipEvents()

    def fused():
        run.batch.flags = 0
        ctx.run_device(run.batch, outs, s)

    def prefix():
        run.batch.flags = abi.BATCH_PREFIXES
        ctx.run_device(run.batch, outs, s)

    def two_pass():
        prefix()
        run.batch.flags = 0
        ctx.resume_device(run.batch, outs, s)

    def decisions():
        ctx.stream_synchronize(s)
        return run.d_dec.download(np.zeros(n, dtype=np.uint8))

    def timed(fn, steps):
        ev.start(s)
        for _ in range(steps):
            fn()
        return ev.stop_ms(s) / steps

    for name, prog in PROGRAMS.items():
        kinds = [abi.KINDS[p.kind] for p in ctx.compile(prog)]
        assert "PAYLOAD" in kinds, kinds
        slot = kinds.index("PAYLOAD")
        # the two forms decide alike, and how many frames the second pass takes
        fused()
        want = decisions()
        prefix()
        first = decisions()
        work = int((first == ((abi.DECIDE_HOST << 6) | slot)).sum())
        two_pass()
        assert np.array_equal(decisions(), want), f"{name}: two-pass decisions differ from the fused pass"
        res = {"fused": [], "prefix": [], "two_pass": []}
        for _ in range(a.rounds):
            for v, fn in (("fused", fused), ("prefix", prefix), ("two_pass", two_pass)):
                timed(fn, 2)   # warm
                res[v].append(timed(fn, a.steps))
        m = {v: med(x) for v, x in res.items()}
        for v in res:
            print(json.dumps({"program": name, "kinds": kinds, "variant": v, "packets": n, "work_items": work,
                              "ms_median": round(m[v], 4), "ms_all": [round(x, 4) for x in sorted(res[v])],
                              "mpps": round(n / (m[v] * 1e-3) / 1e6, 1)}), flush=True)
        print(json.dumps({"program": name, "variant": "resume", "packets": n, "work_items": work,
                          "ms_median": round(m["two_pass"] - m["prefix"], 4),
                          "two_pass_over_fused": round(m["two_pass"] / m["fused"], 3)}), flush=True)
    run.batch.flags = 0
    ctx.stream_destroy(s)
    run.free()


def ring_part(ctx, a):
    n = a.ring_packets
    data, desc0 = synth.capture(synth.C3, n, seed=33)
    ring, rdesc, used = synth.tpv3_ring(data, desc0)
    ring = abi.host_copy(ring)
    desc, rd = abi.host_array(n + 64, np.uint64), abi.host_array(n + 64, np.uint64)
    dec = abi.host_array(n + 64)
    slots = abi.host_array((n + 64) * abi.PREFIX_SLOT)
    held = [ring, desc, rd, dec, slots]
    for x in held:
        ctx.register(x)
    modes = {"in_place": {}, "lean_all": dict(gather=True),
             "lean_all_resume": dict(gather=True, resume_payload=True, ring_desc=rd)}
    try:
        for name, prog in PROGRAMS.items():
            ctx.compile(prog)
            res, left, ref = {m: [] for m in modes}, {}, None
            for r in range(a.rounds + 1):   # round 0 warms
                for m, kw in modes.items():
                    t0 = time.perf_counter()
                    got = abi.ring_stage_tpv3(ctx, ring, synth.TPV3_BLOCK, used, desc, dec, None, slots,
                                              want_host=True, **kw)
                    ms = (time.perf_counter() - t0) * 1e3
                    assert got[0] == n
                    if r:
                        res[m].append(ms)
                    left[m] = got[2]
                    if m == "in_place":
                        ref = dec[:n].copy()
                    elif m == "lean_all_resume":
                        assert np.array_equal(dec[:n], ref), f"{name}: resumed decisions differ from in place"
            for m in modes:
                v = med(res[m])
                print(json.dumps({"program": name, "ring_mode": m, "packets": n, "host_frames_left": left[m],
                                  "ms_median": round(v, 3), "ms_all": [round(x, 3) for x in sorted(res[m])],
                                  "mpps": round(n / (v * 1e-3) / 1e6, 1)}), flush=True)
    finally:
        for x in held:
            ctx.unregister(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ring-packets", type=int, default=1 << 20)
    a = ap.parse_args()
    ctx = abi.Context(0)
    try:
        device_part(ctx, a)
        if a.ring_packets:
            ring_part(ctx, a)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()

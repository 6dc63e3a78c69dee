"""The rate of the PAYLOAD forms that BT_OPT_PAYLOAD_EXTENDED adds: one C3 capture on the
device at the bench's size, the main kernel timed (bt_time_device2 with
BT_TIME_KERNEL_EVENTS, as tools/payload_ab.py does) with one PAYLOAD slot first in C3's
chain, so every IPv4 packet runs it, alternating the variants round by round in one process:

  plain   /GET|POST/            default context: the bit-parallel form (the yardstick)
  wordb   /\\b(GET|POST)\\b/      extended context: a byte DFA with the word-class bit
  wide    /(a|b)*a(a|b){8}/     extended context: the wide form (16-bit state ids)
  wide2   /(ab)*c.{7}d/         extended context: the wide form, a 6 KB table

Without the option the last three stay on the host: a device round trip and a std::regex
per packet that reaches them (the reference's own rate for such a slot is 2.09 Mpps).

Usage: python tools/payload_ext_rate.py [--packets N] [--steps K] [--rounds R]
Prints one JSON line per variant: median main-kernel ms and Mpps, filter only and with records.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from beatrice_amd import abi, synth  # noqa: E402

VARIANTS = {"plain": ("GET|POST", False), "wordb": ("\\b(GET|POST)\\b", True),
            "wide": ("(a|b)*a(a|b){8}", True), "wide2": ("(ab)*c.{7}d", True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ctx = abi.Context(0)
    ext = abi.Context(0, flags=abi.OPT_PAYLOAD_EXTENDED)
    wl = dict(bench.WORKLOADS["c3"], payload="GET|POST")
    cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets)
    run = cap.run
    res, kinds, forms = {}, {}, {}
    for _ in range(a.rounds):
        for v, (expr, extended) in VARIANTS.items():
            c = ext if extended else ctx
            p = c.compile([{"type": abi.PAYLOAD, "expr": expr, "priority": 9}] + bench.C3_FILTERS)
            kinds[v] = abi.KINDS[p[0].kind]
            assert kinds[v] == "PAYLOAD", f"/{expr}/ stayed on the host"
            tag = abi.payload_dfa(expr, abi.DFA_EXTENDED if extended else 0)[:2]
            forms[v] = {b"\xff\xff": "bit-parallel", b"\xfe\xff": "wide DFA"}.get(tag, "byte DFA")
            for rec in (0, 1):
                o = abi.Outputs(run.outs.records if rec else None, run.n, run.outs.verdict, run.outs.decide,
                                run.outs.pass_idx, run.outs.n_pass)
                c.time_device2(run.batch, [o], 2, abi.TIME_KERNEL_EVENTS)   # warm
                t = c.time_device2(run.batch, [o], a.steps, abi.TIME_KERNEL_EVENTS)
                res.setdefault((v, rec), []).append(t.main_ms)
    for v, (expr, extended) in VARIANTS.items():
        for rec in (0, 1):
            ms = sorted(res[(v, rec)])
            med = ms[len(ms) // 2]
            print(json.dumps({"variant": v, "expr": expr, "extended": extended, "form": forms[v], "records": bool(rec),
                              "packets": run.n, "kernel_ms_median": round(med, 4),
                              "kernel_ms_all": [round(x, 4) for x in ms],
                              "mpps": round(run.n / (med * 1e-3) / 1e6, 1)}), flush=True)
    run.free()
    ext.close()
    ctx.close()


if __name__ == "__main__":
    main()

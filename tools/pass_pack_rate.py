"""The rate of the ordered pack (bt_pass_pack_device) and of the pcap filter built on it.

  pack        the bench's C3 capture on the device, the `c3` program's verdict words, packed with
              lead 0 / align 1: both pack kernels between an event pair from their own dispatches
  pack_all    the same capture with all-pass words (every frame is copied) ...
  copy_d2d    ... against one hipMemcpyAsync device-to-device of the same number of output bytes,
              in the same process, alternating round by round: the ceiling for moving those bytes
  pcap        bt_pcap_filter over a pcap of --pcap-bytes synthesised from C3 (wall clock, pinned
              staging, H2D, kernels and D2H included), packets/s and GB/s of input ...
  host_batch  ... against bt_parse_filter over the same frames and descriptors, verdicts only:
              what the packing and the return trip add

Every variant is warmed first; each figure is the median of --rounds rounds, all of them listed.
Usage: python tools/pass_pack_rate.py [--packets N] [--steps K] [--rounds R] [--pcap-bytes B]
Prints one JSON line per variant and a last line with the ratios.
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


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def line(**kw):
    print(json.dumps(kw), flush=True)


def pack_part(ctx, a) -> dict:
    wl = bench.WORKLOADS["c3"]
    cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
    run, n = cap.run, cap.n
    ctx.compile(wl["filters"])
    outs = abi.Outputs(None, n, run.outs.verdict, run.outs.decide, None, None)
    ctx.run_device(run.batch, outs)
    ctx.synchronize()
    lens = synth.desc_len(cap.desc).astype(np.int64)
    words = run.d_ver.download(np.zeros((n + 63) // 64, np.uint64))
    sel = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    all_bytes, sel_bytes = int(lens.sum()), int(lens[sel].sum())
    d_all = ctx.alloc(words.nbytes)
    d_all.upload(np.full(len(words), 0xFFFFFFFFFFFFFFFF, np.uint64))
    d_out, d_tot = ctx.alloc(all_bytes + 256), ctx.alloc(16)
    d_src = ctx.alloc(all_bytes + 256)   # the plain copy's source: as many bytes as pack_all writes
    po = abi.PackOpts(0, 0, 1, 0)
    out = abi.PackOut(d_out.ptr, all_bytes, None, d_tot.ptr, d_tot.ptr + 8)
    ms = (ctypes.c_float * a.steps)()

    def pack(select):
        abi._check(abi.lib().bt_time_pass_pack(ctx.h, ctypes.byref(run.batch), select, ctypes.byref(po),
                                               ctypes.byref(out), a.steps, ms))
        tot = d_tot.download(np.zeros(16, np.uint8))
        return list(ms), int(tot[:8].view(np.uint64)[0]), int(tot[8:12].view(np.uint32)[0])

    def copy():
        abi._check(abi.lib().bt_time_copy_d2d(ctx.h, d_out.ptr, d_src.ptr, all_bytes, a.steps, ms))
        return list(ms)

    variants = {"pack": lambda: pack(run.d_ver.ptr), "pack_all": lambda: pack(d_all.ptr), "copy_d2d": copy}
    for fn in variants.values():   # warm: code objects, the workspace, first touch of the buffers
        fn()
    _, total, packed = pack(run.d_ver.ptr)
    assert (total, packed) == (sel_bytes, int(sel.sum())), (total, packed, sel_bytes, int(sel.sum()))
    _, total, packed = pack(d_all.ptr)
    assert (total, packed) == (all_bytes, n), (total, packed, all_bytes, n)
    res = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v, fn in variants.items():
            r = fn()
            res[v].append(med(r[0] if isinstance(r, tuple) else r))
    m = {v: med(x) for v, x in res.items()}
    moved = {"pack": sel_bytes, "pack_all": all_bytes, "copy_d2d": all_bytes}
    for v in variants:
        line(variant=v, packets=n, selected=int(sel.sum()) if v == "pack" else n, out_bytes=moved[v],
             ms_median=round(m[v], 4), ms_rounds=[round(x, 4) for x in sorted(res[v])],
             out_gbps=round(moved[v] / (m[v] * 1e-3) / 1e9, 1), mpps=round(n / (m[v] * 1e-3) / 1e6, 1))
    for b in (d_all, d_out, d_tot, d_src):
        b.free()
    run.free()
    return {"pack_ms": m["pack"], "pack_all_ms": m["pack_all"], "copy_d2d_ms": m["copy_d2d"],
            "pack_all_over_copy": round(m["pack_all"] / m["copy_d2d"], 3)}


def synth_pcap(n: int, seed: int):
    """A pcap (usec, native order) of n C3 frames: (file bytes, frame data, descriptors)."""
    data, desc = synth.capture(synth.C3, n, seed=seed)
    off, ln = synth.desc_off(desc).astype(np.int64), synth.desc_len(desc).astype(np.int64)
    rec = 24 + np.cumsum(16 + ln) - (16 + ln)   # each record header's offset
    out = np.zeros(int(rec[-1] + 16 + ln[-1]), np.uint8)
    out[:24] = np.frombuffer(np.array([0xA1B2C3D4, 0x00040002, 0, 0, 65535, 1], "<u4").tobytes(), np.uint8)
    hdr = np.zeros((n, 4), "<u4")
    hdr[:, 0], hdr[:, 1], hdr[:, 2], hdr[:, 3] = 1_700_000_000 + np.arange(n) // 1000, np.arange(n) % 1_000_000, ln, ln
    hb = hdr.view(np.uint8).reshape(n, 16)
    step = 1 << 16
    for i in range(0, n, step):
        j = min(n, i + step)
        out[(rec[i:j, None] + np.arange(16)).reshape(-1)] = hb[i:j].reshape(-1)
        k = ln[i:j]
        within = np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k)
        out[np.repeat(rec[i:j] + 16, k) + within] = data[np.repeat(off[i:j], k) + within]
    return out, data, desc


def pcap_part(ctx, a) -> dict:
    n = max(1, a.pcap_bytes // 355)   # C3's mean frame is ~339 B, + 16 B of record header
    pcap, data, desc = synth_pcap(n, seed=41)
    ctx.compile(bench.WORKLOADS["c3"]["filters"])
    out = np.zeros(len(pcap), np.uint8)   # touched: sized for everything passing
    res = abi.PcapResult()
    outs = abi.host_outputs(n, records=False)

    def pcap_filter():
        t0 = time.perf_counter()
        abi._check(abi.lib().bt_pcap_filter(ctx.h, pcap.ctypes.data, len(pcap), out.ctypes.data, len(out),
                                            ctypes.byref(res)))
        return (time.perf_counter() - t0) * 1e3

    def host_batch():
        t0 = time.perf_counter()
        got = ctx.run_host(data, desc, records=False, filters=True, outs=outs)
        ms = (time.perf_counter() - t0) * 1e3
        assert got["n_pass"] == res.n_pass, (got["n_pass"], res.n_pass)
        return ms

    variants = {"pcap": pcap_filter, "host_batch": host_batch}
    for fn in variants.values():   # warm: staging allocation, first touch
        fn()
    assert res.n_in == n and res.n_pass + res.n_reject + res.n_throw == n
    t = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v, fn in variants.items():
            t[v].append(fn())
    m = {v: med(x) for v, x in t.items()}
    for v in variants:
        line(variant=v, packets=n, in_bytes=len(pcap) if v == "pcap" else int(data.nbytes), n_pass=int(res.n_pass),
             out_bytes=int(res.out_bytes) if v == "pcap" else 0, chunks=int(res.chunks) if v == "pcap" else None,
             ms_median=round(m[v], 2), ms_rounds=[round(x, 2) for x in sorted(t[v])],
             mpps=round(n / (m[v] * 1e-3) / 1e6, 2), in_gbps=round(len(pcap) / (m[v] * 1e-3) / 1e9, 2))
    return {"pcap_ms": m["pcap"], "host_batch_ms": m["host_batch"],
            "pcap_over_host_batch": round(m["pcap"] / m["host_batch"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pcap-bytes", type=int, default=1 << 30)
    a = ap.parse_args()
    ctx = abi.Context(0)
    try:
        summary = {}
        if a.packets:
            summary.update(pack_part(ctx, a))
        if a.pcap_bytes:
            summary.update(pcap_part(ctx, a))
        line(summary={k: (round(v, 4) if isinstance(v, float) else v) for k, v in summary.items()})
    finally:
        ctx.close()


if __name__ == "__main__":
    main()

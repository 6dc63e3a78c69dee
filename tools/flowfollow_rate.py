"""The rate of the reassembled-stream export (bt_flow_follow_device) on the bench's C3 capture on the device, and
what the export costs on top of the reassembly.

  follow   bt_flow_follow_device's kernels with --pattern from the first one's start to the last one's end (events
           recorded by the kernels' own dispatches), bytes, runs and place written, and what the time divides
           into: classification + compaction, the first sort, rekey + the second sort, carry scan + join + emit,
           match, the follow's sums + join + emit + runs (sum_ms), its copy (copy_ms), commit. The table is zeroed
           before every launch, so every launch places, sorts, matches and exports every segment. The offsets are
           those of a first bt_flow_tcpseq_device call.
  reasm    bt_flow_reasm_device on the same inputs in the same process; export_ms = follow - reasm.
  plain    bt_flow_follow_device without a pattern; saving_ms = follow - plain.
  pack     bt_pass_pack_device at align 1, lead 0 over the same batch with the delivering packets as `select`
           (place != UINT64_MAX), the yardstick: it copies whole frames in packet order and gathers nothing.
           export_to_pack = export_ms / pack_ms.
  copy     hipMemcpyAsync device to device of `total` bytes.
  Three id patterns: ids=tracker (the tracker's numbers; C3: every packet a flow of its own), ids=rr1024
  (1,024 flows round robin), ids=half_one (half the packets in one flow).

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches, all rounds
listed. Before anything is timed, every output of a prefix of the batch is checked against bt_flow_follow_host,
over two calls.
Usage: python tools/flowfollow_rate.py [--packets N] [--steps K] [--rounds R] [--pattern EXPR] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowfollow/flowfollow_rate.jsonl).
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

PHASES = ("class_ms", "sort_pos_ms", "sort_key_ms", "scan_ms", "match_ms", "sum_ms", "copy_ms", "commit_ms")


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--check-packets", type=int, default=1 << 15)
    ap.add_argument("--pattern", default="GET|POST")
    ap.add_argument("--ids", default="tracker,rr1024,half_one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowfollow", "flowfollow_rate.jsonl"))
    a = ap.parse_args()
    lines = []

    def line(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def stats(r, key="ms"):
        return {key + "_median": round(med(r), 4), key + "_rounds": [round(x, 4) for x in sorted(r)]}

    ctx = abi.Context(0)
    L = abi.lib()
    try:
        blob, _ = abi.flow_stream_compile(a.pattern)
        d_blob = ctx.alloc(len(blob))
        d_blob.upload(blob)
        wl = bench.WORKLOADS["c3"]
        cap = bench.Capture(ctx, wl, a.packets, synth.SEEDS[synth.C3], 0, a.packets, stats=False)
        run, n = cap.run, cap.n
        nw = (n + 63) // 64
        nbytes_all = int(run.batch.bytes)
        ctx.reserve(n)
        one = (ctypes.c_float * 1)()
        ph6, ph8 = (ctypes.c_float * 6)(), (ctypes.c_float * 8)()
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
        abi.Context.flow_track_forget(d_state)
        d_scratch.free()
        d_state.free()
        d_off, d_hit, d_rest, d_rres, d_qres, d_fres = ctx.alloc(8 * n), ctx.alloc(8 * nw), ctx.alloc(8 * nw), ctx.alloc(64), ctx.alloc(64), ctx.alloc(32)
        d_out, d_runs, d_place = ctx.alloc(nbytes_all + 256), ctx.alloc(32 * n), ctx.alloc(8 * n)
        d_sel, d_total, d_npacked = ctx.alloc(8 * nw), ctx.alloc(8), ctx.alloc(8)
        d_work = ctx.alloc(max(abi.flow_follow_scratch_bytes(n, n), abi.flow_tcpseq_scratch_bytes(n, n)))
        routs = abi.FlowReasmOut(d_hit.ptr, d_rest.ptr, d_rres.ptr, (ctypes.c_uint64 * 2)(0, 0))
        fouts = abi.FlowFollowOut(d_out.ptr, nbytes_all, d_runs.ptr, n, 0, d_place.ptr, d_fres.ptr, (ctypes.c_uint64 * 2)(0, 0))

        # right before it is timed: a prefix against the host form, twice into the same tables
        m = min(n, a.check_packets)
        ids = d_id.download(np.zeros(m, np.uint32)) & np.uint32(255)   # 256 flows: long streams in the scan
        desc = np.ascontiguousarray(cap.desc[:m], np.uint64)
        end = int(((desc & np.uint64((1 << 48) - 1)) + (desc >> np.uint64(48))).max())
        nbytes = (end + 15) // 16 * 16
        data = run.d_data.download(np.zeros(nbytes, np.uint8))
        d_qtab, d_tab, d_cid = ctx.alloc(128 * 256), ctx.alloc(128 * 256), ctx.alloc(4 * m)
        d_qtab.zero()
        d_tab.zero()
        d_cid.upload(ids)
        pre = abi.Batch(run.batch.base, run.batch.desc, 0, m, nbytes, run.batch.desc_format, 0)
        hq, host = np.zeros(256, abi.FlowTcpseqRec), np.zeros(256, abi.FlowReasmRec)
        for k in range(2):
            ctx.flow_tcpseq(pre, d_cid, None, 0, d_qtab, 256, d_work, abi.flow_tcpseq_scratch_bytes(m, 256), d_qres, off=d_off)
            ctx.flow_follow(pre, d_cid, None, d_off, 0, blob, d_blob, d_tab, 256, d_work, abi.flow_follow_scratch_bytes(m, 256), d_rres, d_fres,
                            out_bytes=d_out, cap=nbytes, runs=d_runs, run_cap=m, place=d_place, hit=d_hit, rest=d_rest)
            ctx.synchronize()
            hoff, hhit, hrest = np.zeros(m, np.int64), np.zeros((m + 63) // 64, np.uint64), np.zeros((m + 63) // 64, np.uint64)
            hout, hruns, hplace = np.zeros(nbytes, np.uint8), np.zeros(m, abi.FlowFollowRun), np.zeros(m, np.uint64)
            abi.flow_tcpseq_host(data, desc, ids, None, 0, hq, off=hoff)
            hres, hfres = abi.flow_follow_host(data, desc, ids, None, hoff, 0, blob, host, out_bytes=hout, runs=hruns, place=hplace, hit=hhit, rest=hrest)
            fres = abi.FlowFollowResult.from_bytes(d_fres.download(np.zeros(32, np.uint8))).as_dict()
            assert abi.FlowReasmResult.from_bytes(d_rres.download(np.zeros(64, np.uint8))).as_dict() == hres, "the result differs from the host form"
            assert fres == hfres and fres["total"] > 0, "the follow result differs from the host form"
            assert d_tab.download(np.zeros(128 * 256, np.uint8)).tobytes() == host.tobytes(), "the table differs from the host form"
            assert (d_hit.download(np.zeros((m + 63) // 64, np.uint64)) == hhit).all(), "hit differs from the host form"
            assert (d_out.download(np.zeros(fres["written"], np.uint8)) == hout[:fres["written"]]).all(), "the bytes differ from the host form"
            assert d_runs.download(np.zeros(32 * fres["n_runs"], np.uint8)).tobytes() == hruns[:fres["n_runs"]].tobytes(), "the runs differ"
            assert (d_place.download(np.zeros(m, np.uint64)) == hplace).all(), "place differs from the host form"
        for b in (d_qtab, d_tab, d_cid):
            b.free()

        i = np.arange(n, dtype=np.uint32)
        half = np.where(i & 1, np.uint32(0), i).astype(np.uint32)
        variants = {"tracker": (None, nf), "rr1024": (i & np.uint32(1023), 1024), "half_one": (half, n)}
        for name in a.ids.split(","):
            ids, flow_cap = variants[name]
            d_ids = d_id
            if ids is not None:
                d_ids = ctx.alloc(4 * n)
                d_ids.upload(np.ascontiguousarray(ids, np.uint32))
            d_qtab, d_tab = ctx.alloc(128 * flow_cap), ctx.alloc(128 * flow_cap)
            d_qtab.zero()
            qneed, rneed, fneed = abi.flow_tcpseq_scratch_bytes(n, flow_cap), abi.flow_reasm_scratch_bytes(n, flow_cap), abi.flow_follow_scratch_bytes(n, flow_cap)
            ctx.flow_tcpseq(run.batch, d_ids, None, 0, d_qtab, flow_cap, d_work, qneed, d_qres, off=d_off)   # the offsets of a first call
            ctx.synchronize()

            def follow(with_pattern=True):
                d_tab.zero()
                ctx.synchronize()
                abi._check(L.bt_time_flow_follow(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, d_off.ptr, 0,
                                                 blob.ctypes.data if with_pattern else None, d_blob.ptr if with_pattern else None,
                                                 len(blob) if with_pattern else 0, d_tab.ptr, flow_cap, d_work.ptr, fneed, ctypes.byref(routs),
                                                 ctypes.byref(fouts), 1, one, ph8))
                return one[0], list(ph8)

            def reasm():
                d_tab.zero()
                ctx.synchronize()
                abi._check(L.bt_time_flow_reasm(ctx.h, ctypes.byref(run.batch), d_ids.ptr, None, d_off.ptr, 0, blob.ctypes.data, d_blob.ptr,
                                                len(blob), d_tab.ptr, flow_cap, d_work.ptr, rneed, ctypes.byref(routs), 1, one, ph6))
                return one[0], list(ph6)

            def rounds_of(fn, k):
                def rnd():
                    got = [fn() for _ in range(a.steps)]
                    return med([g[0] for g in got]), [med([g[1][j] for g in got]) for j in range(k)]
                rnd()
                rs = [rnd() for _ in range(a.rounds)]
                return [x[0] for x in rs], [round(med([x[1][j] for x in rs]), 4) for j in range(k)]

            f, fph = rounds_of(follow, 8)
            t = abi.FlowReasmResult.from_bytes(d_rres.download(np.zeros(64, np.uint8))).as_dict()
            ft = abi.FlowFollowResult.from_bytes(d_fres.download(np.zeros(32, np.uint8))).as_dict()
            assert t["n"] == n and t["bad_ids"] == 0 and t["late_packets"] == 0 and ft["total"] == t["stream_bytes"] == ft["written"]
            place = d_place.download(np.zeros(n, np.uint64))
            bits = np.zeros(nw * 64, np.uint8)
            bits[:n] = place != np.uint64(0xFFFFFFFFFFFFFFFF)
            d_sel.upload(np.packbits(bits, bitorder="little").view(np.uint64))
            r, rph = rounds_of(reasm, 6)
            p, pph = rounds_of(lambda: follow(False), 8)
            pt = abi.FlowReasmResult.from_bytes(d_rres.download(np.zeros(64, np.uint8))).as_dict()
            assert pt["hit_packets"] == 0 and pt["stream_bytes"] == t["stream_bytes"]

            popts = abi.PackOpts(0, 0, 1, 0)
            pout = abi.PackOut(d_out.ptr, nbytes_all, None, d_total.ptr, d_npacked.ptr)

            def pack():
                abi._check(L.bt_time_pass_pack(ctx.h, ctypes.byref(run.batch), d_sel.ptr, ctypes.byref(popts), ctypes.byref(pout), a.steps, ms))
                return med(list(ms))
            pack()
            pk = [pack() for _ in range(a.rounds)]
            pack_bytes = int(d_total.download(np.zeros(1, np.uint64))[0])

            def copy():
                abi._check(L.bt_time_copy_d2d(ctx.h, d_out.ptr, run.batch.base, max(1, ft["total"]), a.steps, ms))
                return med(list(ms))
            copy()
            cp = [copy() for _ in range(a.rounds)]
            export = med(f) - med(r)
            line(variant="follow", ids=name, packets=n, flow_cap=flow_cap, pattern=a.pattern, stream_packets=t["stream_packets"],
                 total_bytes=ft["total"], n_runs=ft["n_runs"], holes=t["holes"], dup_packets=t["dup_packets"], **stats(f),
                 **dict(zip(PHASES, fph)), reasm_ms=round(med(r), 4), reasm_rounds=[round(x, 4) for x in sorted(r)],
                 export_ms=round(export, 4), pack_ms=round(med(pk), 4), pack_rounds=[round(x, 4) for x in sorted(pk)], pack_bytes=pack_bytes,
                 export_to_pack=round(export / med(pk), 3), follow_phases_to_pack=round((fph[5] + fph[6]) / med(pk), 3),
                 copy_d2d_ms=round(med(cp), 4), copy_to_d2d=round(fph[6] / med(cp), 3),
                 copy_gbps=round(ft["total"] / (fph[6] * 1e-3) / 1e9, 1) if fph[6] > 0 else None,
                 plain_ms=round(med(p), 4), plain_rounds=[round(x, 4) for x in sorted(p)], saving_ms=round(med(f) - med(p), 4),
                 plain_phases=dict(zip(PHASES, pph)), gpps=round(n / (med(f) * 1e-3) / 1e9, 3))
            for b in (d_qtab, d_tab):
                b.free()
            if ids is not None:
                d_ids.free()

        for b in (d_id, d_res, d_off, d_hit, d_rest, d_rres, d_qres, d_fres, d_out, d_runs, d_place, d_sel, d_total, d_npacked, d_work, d_blob):
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

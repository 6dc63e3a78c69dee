"""The rate of the endpoint table over a flow tracker (bt_flow_track_hosts_device) and of what it
replaces, on trackers built from the bench's C3 capture on the device: once with every packet
selected (every packet its own flow) and once with the `c3` program's verdict words as `select`.

  hosts         the call's kernels between an event pair recorded by the first and the last kernel's
                own dispatches, with the side table, host_cap = 2 n_flows and endpoint_host, on four
                tables:
                table=c3        the tracker and the side table as the capture left them
                table=distinct  the records replaced by ones with two fresh hosts per flow
                table=few       ... by ones whose endpoints are drawn from 64 hosts
                table=hub       ... by ones with one address in every flow, the other fresh
  host          what the call replaces (bt_time_flow_hosts_host): the device-to-host copy of the header,
                n_flows records and n_flows side records into pinned memory, then
                bt_flow_track_hosts_host on one thread into host_cap records. It does not write
                endpoint_host, which the device call it is compared with does.
  copy          one hipMemcpyAsync device-to-device of n_flows x 104 bytes: the bytes the call must
                read once

Every variant is warmed first; each figure is the median of --rounds rounds of --steps launches,
all rounds listed. Before a table is timed its outputs are checked: the whole 64-byte result against
the host form's over the downloaded state; six sums over the n_written host records the device wrote
(read back once) against the same sums over the host form's records (packets sent, packets received,
bytes, flows, the state counts weighted by state, stamps with first_flow and syn_packets); the
records' packets sent and received and flows against packets_total and 2 n_flows; n_hosts against
what the table was built to hold; packets_total / bytes_total against the tracker's header (c3) or
numpy (crafted).
Usage: python tools/flowhosts_rate.py [--packets N] [--steps K] [--rounds R] [--select all|verdict] [--out FILE]
Prints one JSON line per variant (also appended to --out, default profiles/flowhosts/flowhosts_rate.jsonl).
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


def record_sums(h: np.ndarray) -> list:
    """bt_time_flow_hosts_host's six sums (mod 2^64) over host records read back from the device."""
    u = np.uint64
    with np.errstate(over="ignore"):
        state = (h["tcp_state"].astype(u) * np.arange(1, 8, dtype=u)).sum(dtype=u)
        mix = h["first_ts"] ^ h["last_ts"] ^ (h["first_flow"].astype(u) << u(32) | h["syn_packets"].astype(u))
        return [int(x) for x in (h["packets"][:, 0].sum(dtype=u), h["packets"][:, 1].sum(dtype=u), (h["bytes"][:, 0] ^ h["bytes"][:, 1]).sum(dtype=u),
                                 h["flows"].astype(u).sum(dtype=u), state, mix.sum(dtype=u))]


def crafted(table: str, nf: int, seed: int):
    """nf BT_FLOW_V4_L4 records whose endpoints follow `table`, with random counts, and their side records."""
    rng = np.random.default_rng(seed)
    f = np.arange(nf, dtype=np.uint32)
    if table == "distinct":
        a, b = np.uint32(0x0A000000) + 2 * f, np.uint32(0x0A000001) + 2 * f
    elif table == "few":
        a, b = np.uint32(0xAC100000) + rng.integers(0, 64, nf, dtype=np.uint32), np.uint32(0xAC100000) + rng.integers(0, 64, nf, dtype=np.uint32)
    else:   # hub: alternating roles
        hub, other = np.full(nf, 0xC0A80001, np.uint32), np.uint32(0x0B000000) + f
        a, b = np.where(f % 2 == 0, hub, other), np.where(f % 2 == 0, other, hub)
    recs = np.zeros(nf, abi.FlowTrackRec)
    recs["key"][:, 0:4] = a.astype(">u4").view(np.uint8).reshape(-1, 4)
    recs["key"][:, 4:8] = b.astype(">u4").view(np.uint8).reshape(-1, 4)
    recs["key"][:, 8:12] = f.view(np.uint8).reshape(-1, 4)   # ports: never part of a host
    recs["klass"] = abi.FLOW_V4_L4
    recs["packets"] = rng.integers(1, 1000, (nf, 2), dtype=np.uint64)
    recs["bytes"] = rng.integers(64, 1 << 20, (nf, 2), dtype=np.uint64)
    recs["first_ts"] = rng.integers(0, 1 << 40, nf, dtype=np.uint64)
    recs["last_ts"] = recs["first_ts"] + rng.integers(0, 1 << 20, nf, dtype=np.uint64)
    tcp = np.zeros(nf, abi.FlowTcpRec)
    tcp["flags"] = rng.choice(np.array([0, 0x02, 0x12, 0x10, 0x11, 0x14, 0x18], np.uint8), (nf, 2))
    tcp["syn_packets"], tcp["fin_packets"] = rng.integers(0, 3, nf, dtype=np.uint32), rng.integers(0, 3, nf, dtype=np.uint32)
    want_hosts = {"distinct": 2 * nf, "few": len(np.unique(np.concatenate([a, b]))), "hub": nf + 1}[table]
    return recs, tcp, want_hosts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--select", choices=("all", "verdict"), default=None, help="one tracker alone")
    ap.add_argument("--tables", default="c3,distinct,few,hub")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowhosts", "flowhosts_rate.jsonl"))
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
        d_scratch, d_res, d_ids, d_tres = ctx.alloc(need), ctx.alloc(64), ctx.alloc(4 * n), ctx.alloc(32)
        for sel_name, sel in (("all", None), ("verdict", run.d_ver.ptr)):
            if a.select and a.select != sel_name:
                continue
            # the tracker: one update of the batch, first with room for every packet, then with room for its flows
            cap_flows = n
            for _ in range(2):
                lay = abi.flow_track_layout(cap_flows)
                d_state, d_tcp = ctx.alloc(lay["total"]), ctx.alloc(16 * cap_flows)
                d_tcp.zero()
                ctx.flow_track_init(d_state, lay["total"], cap_flows)
                ctx.flow_track_update(d_state, run.batch, d_scratch, need, d_res, select=sel, batch_ts=7, flow_id=d_ids)
                ctx.flow_tcp_update(run.batch, d_ids, 0, d_tcp, cap_flows, d_tres)
                ctx.synchronize()
                hdr = abi.FlowTrackHdr.from_bytes(d_state.download(np.zeros(128, np.uint8))).as_dict()
                nf = hdr["n_flows"]
                assert nf and not hdr["overflow_packets"]
                if nf == cap_flows:
                    break
                abi.Context.flow_track_forget(d_state)
                d_state.free()
                d_tcp.free()
                cap_flows = nf
            d_recs = d_state.ptr + lay["records"]
            host_cap = 2 * nf
            hneed = abi.flow_track_hosts_scratch_bytes(cap_flows)
            d_hscratch, d_hres = ctx.alloc(hneed), ctx.alloc(64)
            d_hosts, d_ends = ctx.alloc(128 * host_cap), ctx.alloc(8 * cap_flows)
            opts = abi.FlowHostsOpts(0, host_cap, (ctypes.c_uint32 * 2)(0, 0))
            out = abi.FlowHostsOut(d_hosts.ptr, d_ends.ptr, d_hres.ptr)

            def hosts(steps=a.steps):
                abi._check(L.bt_time_flow_hosts(ctx.h, d_state.ptr, ctypes.byref(opts), d_tcp.ptr, d_hscratch.ptr, hneed, ctypes.byref(out),
                                                steps, ms))
                return list(ms)[:steps]

            moved = 104 * nf
            d_dst = ctx.alloc(moved + 256)

            def copy():
                abi._check(L.bt_time_copy_d2d(ctx.h, d_dst.ptr, d_recs, moved, a.steps, ms))
                return med(list(ms))
            copy()
            cp = stats([copy() for _ in range(a.rounds)])
            line(variant="copy", select=sel_name, bytes=moved, gbps=round(moved / (cp["ms_median"] * 1e-3) / 1e9, 1), **cp)
            d_dst.free()

            for table in a.tables.split(","):
                if table == "c3":
                    want_hosts, want_packets, want_bytes = None, hdr["keyed_packets"], hdr["keyed_bytes"]
                else:   # crafted records and side records under the same header
                    recs, tcp, want_hosts = crafted(table, nf, nf)
                    want_packets = int(recs["packets"].sum(dtype=np.uint64))
                    want_bytes = int(recs["bytes"].sum(dtype=np.uint64))
                    abi._check(L.bt_memcpy_h2d(ctx.h, d_recs, recs.ctypes.data, recs.nbytes))
                    abi._check(L.bt_memcpy_h2d(ctx.h, d_tcp.ptr, tcp.ctypes.data, tcp.nbytes))
                    del recs, tcp
                # what it replaces, and its result for the check
                cms, gms = (ctypes.c_float * a.host_steps)(), (ctypes.c_float * a.host_steps)()
                last, host_sums = abi.FlowHostsResult(), (ctypes.c_uint64 * 6)()
                abi._check(L.bt_time_flow_hosts_host(ctx.h, d_state.ptr, nf, d_tcp.ptr, ctypes.byref(opts), a.host_steps, cms, gms,
                                                     ctypes.byref(last), host_sums))
                both = [c + g for c, g in zip(cms, gms)]
                host = stats(both)
                line(variant="host", select=sel_name, table=table, flows=nf, threads=1, d2h_ms=round(med(list(cms)), 4),
                     group_ms=round(med(list(gms)), 4), **host)
                hosts()   # warm
                res = abi.FlowHostsResult.from_bytes(d_hres.download(np.zeros(64, np.uint8))).as_dict()
                expect(res == last.as_dict(), f"{sel_name} {table}: the device's result {res} differs from the host form's {last.as_dict()}")
                expect(res["status"] == 0 and res["overflow_endpoints"] == 0 and res["n_flows"] == nf, f"{sel_name} {table}: result head")
                expect(want_hosts is None or res["n_hosts"] == want_hosts, f"{sel_name} {table}: n_hosts {res['n_hosts']} != {want_hosts}")
                expect(res["packets_total"] == want_packets and res["bytes_total"] == want_bytes, f"{sel_name} {table}: the totals")
                got = record_sums(d_hosts.download(np.zeros(128 * res["n_written"], np.uint8)).view(abi.FlowHostRec))   # the records themselves
                expect(got == list(host_sums), f"{sel_name} {table}: the device's record sums {got} differ from the host form's {list(host_sums)}")
                expect(res["n_written"] == res["n_hosts"] and got[0] == got[1] == want_packets and got[3] == 2 * nf,
                       f"{sel_name} {table}: the records' packets and flows against the totals")
                r = stats([med(hosts()) for _ in range(a.rounds)])
                line(variant="hosts", select=sel_name, table=table, flows=nf, flow_cap=cap_flows, hosts=res["n_hosts"], slots=res["slots"],
                     scratch_bytes=hneed, **r, gflows=round(nf / (r["ms_median"] * 1e-3) / 1e9, 3),
                     x_copy=round(r["ms_median"] / cp["ms_median"], 2), x_host=round(host["ms_median"] / r["ms_median"], 1))
            abi.Context.flow_track_forget(d_state)
            for b in (d_state, d_tcp, d_hscratch, d_hres, d_hosts, d_ends):
                b.free()
        for b in (d_scratch, d_res, d_ids, d_tres):
            b.free()
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
        raise SystemExit(f"flowhosts_rate: {len(failed)} checks failed")


if __name__ == "__main__":
    main()

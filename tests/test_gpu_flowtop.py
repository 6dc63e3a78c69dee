"""GPU: the top-K query over a device-resident flow tracker (bt_flow_track_top_device,
beatrice_amd/csrc/bt_flowtop.hip). Expected values come from the restatement in flowtop_ref.py
(values from the record fields, np.lexsort over split u64 halves), never from the code under test;
the host form must agree bit for bit. Every output, the result and the scratch sit in poisoned
buffers between two 256-byte guards, the outputs sized to exactly k entries, and are compared
whole; every call runs twice with byte-equal outputs; the state and the side table are read back
unchanged."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowtab_ref as ftr  # noqa: E402
import flowtcp_ref as tr  # noqa: E402
import flowtop_cases as cases  # noqa: E402
import flowtop_ref as top  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_flowtab import POISON, Guarded, Source, golden_keys  # noqa: E402
from test_gpu_flowtcp import packet_tcp  # noqa: E402

pytestmark = pytest.mark.gpu

FLAGS = ftr.BIDIRECTIONAL


class Outs:
    """The outputs of one call of k entries each, the result and the scratch, guarded and poisoned."""

    def __init__(self, ctx, cap, k):
        self.ctx, self.k = ctx, k
        self.need = abi.flow_track_top_scratch_bytes(cap, k)
        self.ids, self.vals, self.recs, self.side = (Guarded(ctx, w * k) for w in (4, 8, 104, 16))
        self.res, self.scratch = Guarded(ctx, 48), Guarded(ctx, self.need)
        self.all = (self.ids, self.vals, self.recs, self.side, self.res, self.scratch)

    def poison(self):
        for g in self.all:
            abi._check(abi.lib().bt_memset_d(self.ctx.h, g.buf.ptr, POISON, g.buf.nbytes))

    def read(self):
        """(result dict, the four outputs' bytes); every guard, the scratch's too, is checked."""
        self.scratch.read()
        return abi.FlowTopResult.from_bytes(self.res.read()).as_dict(), tuple(g.read().tobytes() for g in self.all[:4])

    def free(self):
        for g in self.all:
            g.free()


def check_outputs(got, want, with_tcp, where):
    res, (ids, vals, recs, side) = got
    assert res == want["result"], f"{where}: result {res} != {want['result']}"
    nt = res["n_top"]
    tail = lambda b, w: b[w * nt:] == bytes([POISON]) * (len(b) - w * nt)   # noqa: E731
    assert ids[:4 * nt] == want["top_id"].astype("<u4").tobytes() and tail(ids, 4), f"{where}: top_id"
    assert vals[:8 * nt] == want["top_value"].astype("<u8").tobytes() and tail(vals, 8), f"{where}: top_value"
    assert recs[:104 * nt] == want["top"].tobytes() and tail(recs, 104), f"{where}: top"
    if with_tcp:
        assert side[:16 * nt] == want["top_tcp"].tobytes() and tail(side, 16), f"{where}: top_tcp"
    else:
        assert side == bytes([POISON]) * len(side), f"{where}: top_tcp written without being asked for"


def call_twice(ctx, state, tcp, o, metric, with_tcp, want, where, stream=None):
    """One query into poisoned outputs, twice: both runs equal `want` whole and each other."""
    runs = []
    for _ in range(2):
        o.poison()
        ctx.synchronize()
        ctx.flow_track_top(state, metric, o.k, o.scratch.ptr, o.need, o.res.ptr, top_id=o.ids.ptr, top_value=o.vals.ptr,
                           top=o.recs.ptr, tcp=tcp, top_tcp=o.side.ptr if with_tcp else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        runs.append(o.read())
        check_outputs(runs[-1], want, with_tcp, where)
    assert runs[0] == runs[1], f"{where}: two runs differ"
    return runs[0]


class DevState:
    """An initialised tracker on the device whose header and records are then replaced by crafted ones;
    the slot words stay as the init left them (the query reads header and records only)."""

    def __init__(self, ctx, cap, flags):
        self.ctx, self.cap, self.flags = ctx, cap, flags
        self.lay = abi.flow_track_layout(cap)
        self.state, self.tcp = Guarded(ctx, self.lay["total"]), Guarded(ctx, 16 * cap)
        ctx.flow_track_init(self.state.ptr, self.lay["total"], cap, flags)
        ctx.synchronize()

    def load(self, n_flows, recs, tcp, hdr=None):
        L, h = abi.lib(), self.ctx.h
        hdr = np.frombuffer(hdr or cases.header(self.flags, self.cap, self.lay["slots"], n_flows), np.uint8)
        abi._check(L.bt_memcpy_h2d(h, self.state.ptr, hdr.ctypes.data, 128))
        raw = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
        abi._check(L.bt_memcpy_h2d(h, self.state.ptr + self.lay["records"], raw.ctypes.data, raw.nbytes))
        side = np.ascontiguousarray(tcp).view(np.uint8).reshape(-1)
        abi._check(L.bt_memcpy_h2d(h, self.tcp.ptr, side.ctypes.data, side.nbytes))
        self.ctx.synchronize()
        return self.state.read().tobytes(), self.tcp.read().tobytes()

    def unchanged(self, before):
        return (self.state.read().tobytes(), self.tcp.read().tobytes()) == before

    def free(self):
        abi.Context.flow_track_forget(self.state.ptr)
        self.state.free()
        self.tcp.free()


def host_state(cap, flags, n_flows, recs):
    t = abi.HostFlowTracker(cap, flags)
    t.state[:128] = np.frombuffer(cases.header(flags, cap, t.layout["slots"], n_flows), np.uint8)
    t.state[t.layout["records"]:t.layout["records"] + 104 * cap] = np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    return t


@pytest.mark.parametrize("n_flows", cases.N_FLOWS)
def test_crafted_states(gpu_ctx, n_flows):
    """Every value pattern at this table size, flow_cap == n_flows and above it (garbage behind the live
    records), every k; the metric and whether the side records are asked for rotate."""
    ctx = gpu_ctx
    for cap in cases.caps(n_flows):
        dev = DevState(ctx, cap, FLAGS)
        outs = {k: Outs(ctx, cap, k) for k in cases.ks(n_flows)}
        try:
            for name, metrics, recs, tcp in cases.patterns(n_flows, cap):
                before = dev.load(n_flows, recs, tcp)
                host = host_state(cap, FLAGS, n_flows, recs)
                for metric in metrics:
                    for j, (k, o) in enumerate(outs.items()):
                        where = f"{name} n={n_flows} cap={cap} metric={metric} k={k}"
                        want = top.expected(metric, k, recs[:n_flows], tcp)
                        with_tcp = metric >= top.TCP_SYN or j % 2 == 0
                        got = call_twice(ctx, dev.state.ptr, dev.tcp.ptr if with_tcp else None, o, metric, with_tcp, want, where)
                        hid, hval, hrec, hside, hres = abi.flow_track_top_host(host.state, metric, k, tcp if with_tcp else None)
                        assert hres == got[0] and (hid.tobytes(), hval.tobytes(), hrec.tobytes()) == tuple(
                            b[:w * hres["n_top"]] for b, w in zip(got[1][:3], (4, 8, 104))), f"{where}: the host form"
                        assert not with_tcp or hside.tobytes() == got[1][3][:16 * hres["n_top"]], f"{where}: the host form's side records"
                assert dev.unchanged(before), f"{name} n={n_flows} cap={cap}: the state or the side table was written"
        finally:
            for o in outs.values():
                o.free()
            dev.free()


def test_a_header_that_is_not_this_tracker_gives_status_1_and_nothing_else(gpu_ctx):
    ctx, cap, n = gpu_ctx, 300, 257
    _, _, recs, tcp = cases.patterns(n, cap)[-1]
    dev, o = DevState(ctx, cap, FLAGS), Outs(ctx, cap, 20)
    zero = {"n_flows": 0, "n_top": 0, "status": 1, "metric": 0, "n_ties": 0, "reserved": 0, "threshold": 0, "total": 0, "top_total": 0}
    try:
        slots = dev.lay["slots"]
        for what, hdr in (("magic", b"XXXX" + cases.header(FLAGS, cap, slots, n)[4:]), ("flags", cases.header(0, cap, slots, n)),
                          ("flow_cap", cases.header(FLAGS, cap + 1, slots, n)), ("slots", cases.header(FLAGS, cap, 2 * slots, n)),
                          ("n_flows above flow_cap", cases.header(FLAGS, cap, slots, cap + 1))):
            before = dev.load(n, recs, tcp, hdr=hdr)
            want = {"result": zero, "top_id": np.zeros(0, np.uint32), "top_value": np.zeros(0, np.uint64), "top": recs[:0], "top_tcp": tcp[:0]}
            call_twice(ctx, dev.state.ptr, dev.tcp.ptr, o, top.PACKETS, True, want, what)
            assert dev.unchanged(before)
        before = dev.load(n, recs, tcp)   # the right header again: the same buffers give the top
        call_twice(ctx, dev.state.ptr, dev.tcp.ptr, o, top.PACKETS, True, top.expected(top.PACKETS, 20, recs[:n], tcp), "right header")
        assert dev.unchanged(before)
    finally:
        o.free()
        dev.free()


def test_refusals_that_need_a_known_state(gpu_ctx):
    ctx, cap = gpu_ctx, 64
    dev, o = DevState(ctx, cap, FLAGS), Outs(ctx, cap, 8)
    try:
        for nbytes, k in ((o.need - 1, 8), (abi.flow_track_top_scratch_bytes(cap, 0), 8), (0, 0)):
            with pytest.raises(abi.BtError, match="scratch_bytes"):
                ctx.flow_track_top(dev.state.ptr, top.BYTES, k, o.scratch.ptr, nbytes, o.res.ptr)
        with pytest.raises(abi.BtError, match="TCP metric"):
            ctx.flow_track_top(dev.state.ptr, top.TCP_SYN, 8, o.scratch.ptr, o.need, o.res.ptr)
        abi.Context.flow_track_forget(dev.state.ptr)
        with pytest.raises(abi.BtError, match="not an initialised tracker"):
            ctx.flow_track_top(dev.state.ptr, top.BYTES, 8, o.scratch.ptr, o.need, o.res.ptr)
        ctx.flow_track_init(dev.state.ptr, dev.lay["total"], cap, FLAGS)
        ctx.synchronize()
        assert o.read()[0]["n_flows"] == 0xC7C7C7C7   # no refused call wrote anything
    finally:
        o.free()
        dev.free()


@pytest.mark.parametrize("name,cap", [("c3", 5000), ("fuzz", 700)])
def test_end_to_end_behind_the_updates_on_one_stream(gpu_ctx, name, cap):
    """A golden and half of it again through bt_flow_track_update_device in 3 batches with the side table
    behind each, on one non-default stream, and the five queries enqueued behind them with no wait
    in between; against the restatement over flowtrack_ref / flowtcp_ref."""
    ctx = gpu_ctx
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    n = n0 + n0 // 2
    desc, reps = np.resize(g["desc"], n), np.resize(np.arange(n0), n)
    keys = golden_keys(name, False)
    tcp, fl, dirs = packet_tcp(name, False, FLAGS)
    ref, want_tcp = fkr.Tracker(cap, FLAGS), np.zeros(cap, tr.TCP_REC)
    dev = DevState(ctx, cap, FLAGS)
    abi._check(abi.lib().bt_memset_d(ctx.h, dev.tcp.ptr, 0, 16 * cap))
    ctx.synchronize()
    k = 20
    outs = [Outs(ctx, cap, k) for _ in top.METRICS]
    st = ctx.stream_create()
    bufs, srcs, idbufs = [], [], []
    try:
        bounds = np.linspace(0, n, 4).astype(int)
        for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            r = reps[lo:hi]
            src = Source(ctx, name, hi - lo, "packed", desc=desc[lo:hi])
            need = abi.flow_track_scratch_bytes(hi - lo)
            ids, res, scratch, tres = Guarded(ctx, 4 * (hi - lo)), Guarded(ctx, 64), Guarded(ctx, need), Guarded(ctx, 32)
            srcs.append(src)
            bufs += [ids, res, scratch, tres]
            wid = ref.update(keys[0][r], keys[1][r], keys[2][r], src.lens, None, None, 10 * b)["flow_id"]
            tr.update(want_tcp, wid, tcp[r], fl[r], dirs[r])
            idbufs.append((ids, wid))
            ctx.flow_track_update(dev.state.ptr, src.batch, scratch.ptr, need, res.ptr, batch_ts=10 * b, flow_id=ids.ptr, stream=st)
            ctx.flow_tcp_update(src.batch, ids.ptr, FLAGS, dev.tcp.ptr, cap, tres.ptr, stream=st)
        for metric, o in zip(top.METRICS, outs):
            ctx.flow_track_top(dev.state.ptr, metric, k, o.scratch.ptr, o.need, o.res.ptr, top_id=o.ids.ptr, top_value=o.vals.ptr,
                               top=o.recs.ptr, tcp=dev.tcp.ptr, top_tcp=o.side.ptr, stream=st)
        ctx.stream_synchronize(st)
        ctx.synchronize()
        for ids, wid in idbufs:
            assert (ids.read(np.uint32) == wid).all()
        recs = ref.records()
        assert len(recs) > k and (cap > len(recs) or ref.header()["overflow_packets"] > 0)
        for metric, o in zip(top.METRICS, outs):
            check_outputs(o.read(), top.expected(metric, k, recs, want_tcp), True, f"{name} metric={metric}")
        assert dev.tcp.read().tobytes() == want_tcp.tobytes()
        raw = dev.state.read()
        assert raw[dev.lay["records"]:dev.lay["records"] + 104 * cap].tobytes() == ref.records(whole=True).tobytes()
    finally:
        ctx.stream_destroy(st)
        for b in bufs + srcs + outs:
            b.free()
        dev.free()

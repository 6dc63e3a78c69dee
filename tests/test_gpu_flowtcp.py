"""GPU: the per-flow TCP side table (bt_flow_tcp_update_device, beatrice_amd/csrc/bt_flowtcp.hip) and
the tracker's TCP-aware expire (bt_flow_track_expire_tcp_device). Expected values come from the
restatement in flowtcp_ref.py (flags, ok and fragment bits from the goldens' reference-made bt_rec,
or the Python layer walk for cut and crafted frames; keys through flow_ref and flowtab_ref), never
from the code under test; the host form must agree bit for bit. The side table and the result sit
in poisoned buffers between two 256-byte guards and are compared whole."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
import flowtcp_ref as tr  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_gpu_flowtab import FORMATS, POISON, SIZES, SOURCES, Guarded, Source, golden_keys, select_words, strided  # noqa: E402

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
ALL_FLAGS = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)


@functools.lru_cache(maxsize=None)
def packet_tcp(name, fmt_stride, flags):
    """Per frame of a golden (cut to the fixed stride or whole): (contributes, flags byte, direction)."""
    l3 = bool(flags & ftr.L3_ONLY)
    if fmt_stride:
        rows, keys = strided(name)
        tcp, fl = tr.tcp_of_frames([r.tobytes() for r in rows])
        return tcp, fl, tr.directions(*keys[l3], flags)
    g, _ = load_golden(name)
    tcp, fl = tr.tcp_of_rec(g["rec"])
    return tcp, fl, tr.directions(*golden_keys(name, l3), flags)


def tcp_call(ctx, batch, n, d_ids, flags, cap, want_table, want_res, start=None, stream=None, where=""):
    """One bt_flow_tcp_update_device into a guarded side table (zero, or `start`) and a guarded
    result, twice: both runs equal `want` whole and each other. Returns the table's bytes."""
    outs = []
    for _ in range(2):
        tcp, res = Guarded(ctx, 16 * cap), Guarded(ctx, 32)
        try:
            if cap:
                if start is None:
                    abi._check(abi.lib().bt_memset_d(ctx.h, tcp.ptr, 0, 16 * cap))
                else:
                    abi._check(abi.lib().bt_memcpy_h2d(ctx.h, tcp.ptr, start.ctypes.data, 16 * cap))
            ctx.synchronize()
            ctx.flow_tcp_update(batch, d_ids, flags, tcp.ptr if cap else None, cap, res.ptr, stream=stream)
            if stream is not None:
                ctx.stream_synchronize(stream)
            ctx.synchronize()
            got = abi.FlowTcpResult.from_bytes(res.read()).as_dict()
            assert got == want_res, f"{where}: result {got} != {want_res}"
            table = tcp.read()   # its guards: nothing is written outside tcp[0 .. flow_cap)
            bad = np.nonzero(table.view(np.uint32) != want_table.view(np.uint32).reshape(-1))[0]
            assert len(bad) == 0, f"{where}: side table differs at words {bad[:8]} (record {bad[:8] // 4})"
            outs.append(table.tobytes())
        finally:
            tcp.free()
            res.free()
    assert outs[0] == outs[1]
    return outs[0]


def upload(ctx, arr):
    d = ctx.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        d.upload(arr)
    return d


def golden_case(ctx, name, n, fmt, flags, kind, where, stream=None):
    """A golden repeated to n packets: the per-batch table numbers the packets on the device, the side
    table follows on the same stream; the expected ids and table come from the restatements."""
    src = Source(ctx, name, n, fmt)
    sel = select_words(kind, n)
    d_sel = upload(ctx, sel) if sel is not None else None
    ids, scratch, fres = Guarded(ctx, 4 * n), Guarded(ctx, abi.flow_table_scratch_bytes(n, 0)), Guarded(ctx, 72)
    try:
        want_ids = src.want(flags, sel)["flow_id"]
        tcp, fl, dirs = packet_tcp(name, fmt == "stride", flags)
        r = src.reps
        want = np.zeros(n, tr.TCP_REC)
        want_res = tr.update(want, want_ids, tcp[r], fl[r], dirs[r])
        ctx.flow_table_device(src.batch, abi.FlowTableOpts(flags, 0, 0, 0), scratch.ptr, scratch.size, fres.ptr, select=d_sel,
                              flow_id=ids.ptr, stream=stream)
        got = tcp_call(ctx, src.batch, n, ids.ptr, flags, n, want, want_res, stream=stream, where=where)
        assert (ids.read(np.uint32) == want_ids).all(), f"{where}: the table's flow ids"
        if fmt == "packed" and n:   # the host form, bit for bit
            host = np.zeros(n, abi.FlowTcpRec)
            g, _ = load_golden(name)
            assert abi.flow_tcp_update_host(g["data"], src.desc, want_ids, flags, host) == want_res
            assert host.tobytes() == got
        return want_res
    finally:
        for b in (ids, scratch, fres, src) + ((d_sel,) if d_sel is not None else ()):
            b.free()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_chunk_edges(gpu_ctx, n):
    """c3 cycled to every size, so that flows span waves, blocks and chunks; the format, the flags and the selection rotate."""
    si = SIZES.index(n)
    res = golden_case(gpu_ctx, "c3", n, FORMATS[si % 3], ALL_FLAGS[si % 4], ("null", "random")[si % 2], f"c3 n={n}")
    assert res["n"] == n and (n < 63 or res["tcp_packets"] > 0)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", SOURCES)
def test_sources_in_every_format(gpu_ctx, name, fmt):
    """Each golden repeated two and a half times, on a stream of its own."""
    g, _ = load_golden(name)
    n = len(g["desc"]) * 5 // 2
    k = SOURCES.index(name) + FORMATS.index(fmt)
    st = gpu_ctx.stream_create()
    try:
        res = golden_case(gpu_ctx, name, n, fmt, ALL_FLAGS[(k + 1) % 4], ("random", "null")[k % 2], f"{name} {fmt}", stream=st)
        assert res["tcp_packets"] > 0 and (name == "edge" or (res["syn_packets"] > 0 and res["fin_packets"] > 0))
    finally:
        gpu_ctx.stream_destroy(st)


def _frame64(src, dst, sp, dp, flags):
    """A 64-byte IPv4 / TCP frame."""
    ip = bytes([0x45, 0, 0, 50, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + bytes([0x50, flags]) + bytes(6) + bytes(10)


def crafted(ctx, frames, ids, flags, cap, where, start=None):
    """64-byte frames at a fixed stride with the caller's flow ids; the restatement from the Python walk."""
    assert all(len(f) == 64 for f in frames)
    n = len(frames)
    d = upload(ctx, np.frombuffer(b"".join(frames), np.uint8))
    d_ids = upload(ctx, np.asarray(ids, np.uint32))
    try:
        tcp, fl = tr.tcp_of_frames(frames)
        dirs = tr.directions(*fr.key_of_frames(frames, bool(flags & ftr.L3_ONLY)), flags)
        want = np.zeros(cap, tr.TCP_REC) if start is None else start.copy()
        want_res = tr.update(want, ids, tcp, fl, dirs)
        tcp_call(ctx, abi.Batch(d.ptr, None, 64, n, 0, 0, 0), n, d_ids.ptr, flags, cap, want, want_res, start=start, where=where)
        return want, want_res
    finally:
        d.free()
        d_ids.free()


A, B = [10, 0, 0, 1], [10, 0, 0, 2]


def test_one_flow_of_16385_packets_alternating_directions(gpu_ctx):
    """Every packet on one record: the most contention there is, and after the first tiles every
    flag bit is already set, so the pre-read path decides. The flag bytes cycle through all 256."""
    n = 16385
    frames = [_frame64(A, B, 1000, 80, i & 255) if i % 2 == 0 else _frame64(B, A, 80, 1000, (i * 7) & 255) for i in range(n)]
    want, res = crafted(gpu_ctx, frames, np.zeros(n, np.uint32), ftr.BIDIRECTIONAL, 1, "one flow")
    assert res["tcp_packets"] == n and want["flags"].tolist() == [[0xFE, 0xFF]] and int(want["fin_packets"][0]) == n // 2
    # the same packets onto a record that already holds every bit and counters near 2^32: they wrap
    start = np.zeros(1, tr.TCP_REC)
    start["flags"], start["syn_packets"], start["rst_packets"] = [0xFF, 0xFF], 0xFFFFFFF0, 0xFFFFFFFF
    want, _ = crafted(gpu_ctx, frames[:4097], np.zeros(4097, np.uint32), ftr.BIDIRECTIONAL, 1, "one flow, bits set", start=start)
    assert int(want["syn_packets"][0]) < 0xFFFFFFF0 and int(want["rst_packets"][0]) < 0xFFFFFFFF


def test_64_distinct_flows_in_one_tile_and_ids_that_are_not_flows(gpu_ctx):
    frames = [_frame64([10, 1, 0, k], B, 2000 + k, 443, (k * 5 + 2) & 255) for k in range(64)]
    ids = np.arange(64, dtype=np.uint32)[::-1].copy()
    want, res = crafted(gpu_ctx, frames, ids, 0, 64, "64 flows")
    assert res["tcp_packets"] == 64 and (want["flags"][:, 0] != 0).all()
    # sentinels contribute nothing and are not counted; 0xFFFFFFFC and ids at or past flow_cap are bad ids
    ids = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 0xFFFFFFFC, 5, 6, 4] + [4] * 54, np.uint32)
    want, res = crafted(gpu_ctx, frames, ids, ftr.BIDIRECTIONAL, 5, "sentinels and bad ids")
    assert res["bad_ids"] == 3 and res["tcp_packets"] == 57
    _, res = crafted(gpu_ctx, frames, np.arange(64, dtype=np.uint32), 0, 0, "flow_cap 0")
    assert res == {"n": 64, "tcp_packets": 0, "syn_packets": 0, "fin_packets": 0, "rst_packets": 0, "bad_ids": 64, "reserved": [0, 0]}


def test_bytes_cutting_the_last_frames_tcp_header(gpu_ctx):
    """The frame sits at offset 17: its TCP flags byte is byte 64 of the buffer, its protocol byte 40.
    bytes = 80: whole. 64: the TCP layer is still parsed from the length, the flags byte reads as
    zero. 32: the protocol byte reads as zero, and the packet stops contributing, exactly as the
    parser's record loses BT_L_TCP. (The buffer is 16-byte aligned: the read rule cuts at `bytes`.)"""
    frame = _frame64(A, B, 1000, 80, tr.SYN | tr.FIN)
    data = np.zeros(96, np.uint8)
    data[17:17 + 64] = np.frombuffer(frame, np.uint8)
    desc = np.array([17 | 64 << 48], np.uint64)
    for nbytes, contributes in ((80, True), (64, True), (32, False)):
        seen = bytes(data[:nbytes]) + bytes(96 - nbytes)
        tcp, fl = tr.tcp_of_frames([seen[17:17 + 64]])
        assert bool(tcp[0]) == contributes and int(fl[0]) == (tr.SYN | tr.FIN if nbytes == 80 else 0)
        src = Source(gpu_ctx, "edge", 1, "packed", data=data, desc=desc, nbytes=nbytes)
        d_ids = upload(gpu_ctx, np.zeros(1, np.uint32))
        try:
            assert src.d_data.ptr % 16 == 0
            want = np.zeros(1, tr.TCP_REC)
            want_res = tr.update(want, [0], tcp, fl, [0])
            got = tcp_call(gpu_ctx, src.batch, 1, d_ids.ptr, 0, 1, want, want_res, where=f"bytes={nbytes}")
            host = np.zeros(1, abi.FlowTcpRec)
            assert abi.flow_tcp_update_host(data, desc, [0], 0, host, nbytes=nbytes) == want_res and host.tobytes() == got
        finally:
            src.free()
            d_ids.free()


class DevTcpTracker:
    """A tracker and its side table on the device, the restatement and the host form side by side.
    Every call is prepared first (buffers, uploads, what it must give), then all of them are
    enqueued back to back and waited for once."""

    def __init__(self, ctx, flow_cap, flags):
        self.ctx, self.cap, self.flags = ctx, flow_cap, flags
        self.layout = abi.flow_track_layout(flow_cap)
        self.state, self.tcp = Guarded(ctx, self.layout["total"]), Guarded(ctx, 16 * flow_cap)
        abi._check(abi.lib().bt_memset_d(ctx.h, self.tcp.ptr, 0, 16 * flow_cap))
        self.ref, self.want = fkr.Tracker(flow_cap, flags), np.zeros(flow_cap, tr.TCP_REC)
        self.host = abi.HostFlowTracker(flow_cap, flags)
        self.calls, self.checks, self.bufs = [], [], []

    def update(self, src, keys, tcp, fl, dirs, host_data, batch_ts, where):
        ctx, n = self.ctx, src.n
        need = abi.flow_track_scratch_bytes(n)
        ids, res, scratch, tres = Guarded(ctx, 4 * n), Guarded(ctx, 64), Guarded(ctx, need), Guarded(ctx, 32)
        self.bufs += [ids, res, scratch, tres]
        want_ids = self.ref.update(keys[0], keys[1], keys[2], src.lens, None, None, batch_ts)["flow_id"]
        want_res = tr.update(self.want, want_ids, tcp, fl, dirs)
        hid, _ = self.host.update(host_data, src.desc, batch_ts=batch_ts)
        assert self.host.tcp_update(host_data, src.desc, hid) == want_res and (hid == want_ids).all()

        def call():
            ctx.flow_track_update(self.state.ptr, src.batch, scratch.ptr, need, res.ptr, batch_ts=batch_ts, flow_id=ids.ptr)
            ctx.flow_tcp_update(src.batch, ids.ptr, self.flags, self.tcp.ptr, self.cap, tres.ptr)

        def check():
            assert (ids.read(np.uint32) == want_ids).all(), f"{where}: flow ids"
            assert abi.FlowTcpResult.from_bytes(tres.read()).as_dict() == want_res, f"{where}: result"
            scratch.read()
        self.calls.append(call)
        self.checks.append(check)
        return want_ids

    def expire(self, now, idle, closed_idle, expired_cap, where, plain=False):
        ctx, cap = self.ctx, self.cap
        need = abi.flow_track_expire_scratch_bytes(cap) if plain else abi.flow_track_expire_tcp_scratch_bytes(cap)
        exp, exp_tcp, remap = Guarded(ctx, 104 * expired_cap), Guarded(ctx, 16 * expired_cap), Guarded(ctx, 4 * cap)
        res, scratch = Guarded(ctx, 32), Guarded(ctx, need)
        self.bufs += [exp, exp_tcp, remap, res, scratch]
        want = tr.expire(self.ref, self.want, now, idle, closed_idle, expired_cap)
        hexp, hexp_tcp, hremap, hres = self.host.expire_tcp(now, idle, closed_idle, expired_cap)

        def call():
            if plain:
                ctx.flow_track_expire(self.state.ptr, now, idle, scratch.ptr, need, res.ptr, expired=exp.ptr, expired_cap=expired_cap,
                                      remap=remap.ptr)
            else:
                ctx.flow_track_expire_tcp(self.state.ptr, now, idle, closed_idle, self.tcp.ptr, scratch.ptr, need, res.ptr,
                                          expired=exp.ptr, expired_cap=expired_cap, expired_tcp=exp_tcp.ptr, remap=remap.ptr)
        out = {}

        def check():
            got = abi.FlowTrackExpireResult.from_bytes(res.read()).as_dict()
            assert got == want["result"] == hres, f"{where}: expire result {got} != {want['result']}"
            nb, ne = got["n_flows_before"], got["n_expired"]
            rm = remap.read(np.uint32)
            assert (rm[:nb] == want["remap"]).all() and (rm[:nb] == hremap[:nb]).all(), f"{where}: remap"
            assert (rm[nb:] == np.uint32(0x01010101 * POISON)).all(), f"{where}: remap written at or past n_flows_before"
            e = exp.read()
            assert e[:104 * ne].tobytes() == want["expired"].tobytes() == hexp.tobytes() and (e[104 * ne:] == POISON).all(), f"{where}: expired"
            et = exp_tcp.read()
            if not plain:
                assert et[:16 * ne].tobytes() == want["expired_tcp"].tobytes() == hexp_tcp.tobytes(), f"{where}: expired_tcp"
            assert (et[16 * (0 if plain else ne):] == POISON).all(), f"{where}: expired_tcp written at or past n_expired"
            scratch.read()
            out.update(result=got, remap=rm[:nb].copy(), expired=e[:104 * ne].tobytes())
        self.calls.append(call)
        self.checks.append(check)
        return out

    def finish(self, side_table=True):
        ctx = self.ctx
        ctx.synchronize()
        ctx.flow_track_init(self.state.ptr, self.layout["total"], self.cap, self.flags)
        for call in self.calls:
            call()
        ctx.synchronize()
        for check in self.checks:
            check()
        raw, lay = self.state.read(), self.layout
        hdr = abi.FlowTrackHdr.from_bytes(raw).as_dict()
        assert hdr == self.ref.header() == self.host.header()
        recs = raw[lay["records"]:lay["records"] + 104 * self.cap]
        assert recs.tobytes() == self.ref.records(whole=True).tobytes()
        assert self.host.state[lay["records"]:lay["records"] + 104 * self.cap].tobytes() == recs.tobytes()
        table = self.tcp.read()
        if side_table:
            assert table.tobytes() == self.want.tobytes() == self.host.tcp_table().tobytes(), "the side table"
        return raw[:128].tobytes() + recs.tobytes(), table.tobytes()

    def free(self):
        abi.Context.flow_track_forget(self.state.ptr)
        for b in self.bufs + [self.state, self.tcp]:
            b.free()


def tracked(ctx, name, flags, cap, batches, expire_at, plain=False, closed_idle=3):
    """Batches of a golden through a tracker with a small flow_cap (an overflow), the side table
    behind each, one expire in between, more batches. batch b is stamped 10 b."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    l3 = bool(flags & ftr.L3_ONLY)
    keys = golden_keys(name, l3)
    tcp, fl, dirs = packet_tcp(name, False, flags)
    t = DevTcpTracker(ctx, cap, flags)
    srcs, out = [], None
    try:
        for b, (n, start) in enumerate(batches):
            if b == expire_at:   # flows last seen in batch 0 are idle; closed and reset ones seen in batch 1 leave too
                out = t.expire(10 * b, 15, U64_MAX if plain else closed_idle, cap, f"{name} expire", plain=plain)
            reps = (start + np.arange(n)) % n0
            src = Source(ctx, name, n, "packed", desc=g["desc"][reps])
            srcs.append(src)
            ids = t.update(src, (keys[0][reps], keys[1][reps], keys[2][reps]), tcp[reps], fl[reps], dirs[reps], g["data"], 10 * b,
                           f"{name} batch {b}")
        state, table = t.finish(side_table=not plain)
        return state, table, out, t.ref, ids
    finally:
        t.free()
        for s in srcs:
            s.free()


BATCHES = [(700, 0), (65, 650), (16385, 300), (64, 0)]


@pytest.mark.parametrize("name,flags,cap", [("c4", ftr.BIDIRECTIONAL, 900), ("fuzz", 0, 400), ("c3", ftr.L3_ONLY | ftr.BIDIRECTIONAL, 4096)])
def test_ids_from_a_tracker_with_an_overflow_and_an_expire_in_between(gpu_ctx, name, flags, cap):
    state, table, out, ref, ids = tracked(gpu_ctx, name, flags, cap, BATCHES, 2)
    again = tracked(gpu_ctx, name, flags, cap, BATCHES, 2)
    assert (state, table) == again[:2]   # two runs byte-equal
    r = out["result"]
    assert r["n_expired"] > 0 and r["n_flows"] > 0
    if cap < 4096:
        assert ref.header()["overflow_packets"] > 0 and (ids == abi.FLOW_ID_OVERFLOW).any()
    assert r["n_idle"] == r["n_expired"]   # expired_cap = flow_cap: room for all


def test_expire_tcp_that_never_applies_equals_the_plain_expire(gpu_ctx):
    """closed_idle = 2^64 - 1 on the device: state, remap, expired and result byte-equal to bt_flow_track_expire_device."""
    a = tracked(gpu_ctx, "c4", ftr.BIDIRECTIONAL, 900, BATCHES, 2, closed_idle=U64_MAX)
    b = tracked(gpu_ctx, "c4", ftr.BIDIRECTIONAL, 900, BATCHES, 2, plain=True)
    assert a[0] == b[0]
    for k in ("result", "expired"):
        assert a[2][k] == b[2][k]
    assert (a[2]["remap"] == b[2]["remap"]).all() and a[2]["result"]["n_expired"] > 0
    short = tracked(gpu_ctx, "c4", ftr.BIDIRECTIONAL, 900, BATCHES, 2)
    assert short[2]["result"]["n_idle"] > a[2]["result"]["n_idle"]   # closed connections leave earlier with a short closed_idle

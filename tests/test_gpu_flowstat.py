"""GPU: the per-flow statistics side table (bt_flow_stat_update_device, beatrice_amd/csrc/bt_flowstat.hip)
and the generic side-table move behind an expire (bt_flow_track_side_move_device). Expected values
come from the restatement in flowstat_ref.py (a Python layer walk over the frames' bytes; keys
through flow_ref and flowtab_ref), never from the code under test; the host form must agree bit
for bit. The side table and the result sit in poisoned buffers between two 256-byte guards and are
compared whole; every call is made twice and the two runs must be byte-equal."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flowstat_ref as sr  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
import flowtcp_ref as tr  # noqa: E402
import flowtrack_ref as fkr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402
from flowstat_cases import arithmetic_frames, ip4, pack_frames, tcp_hdr  # noqa: E402
from test_gpu_flowtab import FORMATS, POISON, SIZES, SOURCES, Guarded, Source, golden_keys, select_words, strided  # noqa: E402

pytestmark = pytest.mark.gpu

U64_MAX = (1 << 64) - 1
ALL_FLAGS = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)
REC = 128


@functools.lru_cache(maxsize=None)
def packet_facts(name, fmt_stride):
    """What every frame of a golden (cut or padded to the fixed stride, or whole) contributes, by the Python walk."""
    if fmt_stride:
        return sr.facts_of_frames([r.tobytes() for r in strided(name)[0]])
    g, _ = load_golden(name)
    off, ln = (g["desc"] & fr.MASK48).astype(np.int64), (g["desc"] >> np.uint64(48)).astype(np.int64)
    return sr.facts_of_frames([g["data"][o:o + m].tobytes() for o, m in zip(off, ln)])


@functools.lru_cache(maxsize=None)
def packet_dirs(name, fmt_stride, flags):
    l3 = bool(flags & ftr.L3_ONLY)
    return tr.directions(*(strided(name)[1][l3] if fmt_stride else golden_keys(name, l3)), flags)


def stamps(n, seed):
    """Per-packet timestamps that are not in order."""
    return np.uint64(1000) + np.random.default_rng(seed).integers(0, 5000, n).astype(np.uint64)


def upload(ctx, arr):
    d = ctx.alloc(max(16, arr.nbytes))
    if arr.nbytes:
        d.upload(arr)
    return d


def stat_call(ctx, batch, d_ids, flags, cap, want_table, want_res, ts=None, batch_ts=0, start=None, stream=None, where=""):
    """One bt_flow_stat_update_device into a guarded side table (zero, or `start`) and a guarded
    result, twice: both runs equal `want` whole and each other. Returns the table's bytes."""
    outs = []
    d_ts = upload(ctx, np.asarray(ts, np.uint64)) if ts is not None else None
    try:
        for _ in range(2):
            stat, res = Guarded(ctx, REC * cap), Guarded(ctx, 32)
            try:
                if cap:
                    if start is None:
                        abi._check(abi.lib().bt_memset_d(ctx.h, stat.ptr, 0, REC * cap))
                    else:
                        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, stat.ptr, start.ctypes.data, REC * cap))
                ctx.synchronize()
                ctx.flow_stat_update(batch, d_ids, flags, stat.ptr if cap else None, cap, res.ptr, ts=d_ts, batch_ts=batch_ts, stream=stream)
                if stream is not None:
                    ctx.stream_synchronize(stream)
                ctx.synchronize()
                got = abi.FlowStatResult.from_bytes(res.read()).as_dict()
                assert got == want_res, f"{where}: result {got} != {want_res}"
                table = stat.read()   # its guards: nothing is written outside stat[0 .. flow_cap)
                bad = np.nonzero(table.view(np.uint32) != want_table.view(np.uint32).reshape(-1))[0]
                assert len(bad) == 0, f"{where}: side table differs at words {bad[:8]} (record {bad[:8] // 32}, word {bad[:8] % 32})"
                outs.append(table.tobytes())
            finally:
                stat.free()
                res.free()
    finally:
        if d_ts is not None:
            d_ts.free()
    assert outs[0] == outs[1]
    return outs[0]


def golden_case(ctx, name, n, fmt, flags, kind, per_packet_ts, where, stream=None):
    """A golden repeated to n packets: the per-batch table numbers the packets on the device, the side
    table follows on the same stream; the expected ids and table come from the restatements."""
    src = Source(ctx, name, n, fmt)
    sel = select_words(kind, n)
    d_sel = upload(ctx, sel) if sel is not None else None
    ids, scratch, fres = Guarded(ctx, 4 * n), Guarded(ctx, abi.flow_table_scratch_bytes(n, 0)), Guarded(ctx, 72)
    try:
        want_ids = src.want(flags, sel)["flow_id"]
        facts, dirs = packet_facts(name, fmt == "stride"), packet_dirs(name, fmt == "stride", flags)
        r = src.reps
        ts = stamps(n, n) if per_packet_ts and n else None
        want = np.zeros(n, sr.STAT_REC)
        want_res = sr.update(want, want_ids, facts[r], dirs[r], 4242 if ts is None else ts)
        ctx.flow_table_device(src.batch, abi.FlowTableOpts(flags, 0, 0, 0), scratch.ptr, scratch.size, fres.ptr, select=d_sel,
                              flow_id=ids.ptr, stream=stream)
        got = stat_call(ctx, src.batch, ids.ptr, flags, n, want, want_res, ts=ts, batch_ts=4242, stream=stream, where=where)
        assert (ids.read(np.uint32) == want_ids).all(), f"{where}: the table's flow ids"
        if fmt == "packed" and n:   # the host form, bit for bit
            host = np.zeros(n, abi.FlowStatRec)
            g, _ = load_golden(name)
            assert abi.flow_stat_update_host(g["data"], src.desc, want_ids, flags, host, ts=ts, batch_ts=4242) == want_res
            assert host.tobytes() == got
        return want_res
    finally:
        for b in (ids, scratch, fres, src) + ((d_sel,) if d_sel is not None else ()):
            b.free()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_chunk_edges(gpu_ctx, n):
    """c3 cycled to every size, so that flows span waves, blocks and chunks; the format, the flags and
    the selection rotate; per-packet stamps on the odd cases, the batch's stamp alone on the even ones."""
    si = SIZES.index(n)
    res = golden_case(gpu_ctx, "c3", n, FORMATS[si % 3], ALL_FLAGS[si % 4], ("null", "random")[si % 2], si % 2 == 1, f"c3 n={n}")
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
        res = golden_case(gpu_ctx, name, n, fmt, ALL_FLAGS[(k + 1) % 4], ("random", "null")[k % 2], k % 2 == 0, f"{name} {fmt}", stream=st)
        assert res["ip_packets"] >= res["l4_packets"] >= res["tcp_packets"] > 0
    finally:
        gpu_ctx.stream_destroy(st)


A, B = [10, 0, 0, 1], [10, 0, 0, 2]


def slot64(src, dst, sp, dp, fl, ttl=64, length=64, payload=10):
    """An IPv4 / TCP frame of `length` bytes (54 .. 64) in a 64-byte slot; total_length says `payload` bytes of payload."""
    f = ip4(6, tcp_hdr(sp, dp, fl), src, dst, ttl=ttl, total=40 + payload)
    return f + bytes(length - len(f)), length


def crafted(ctx, slots, ids, flags, cap, where, ts=None, batch_ts=0, start=None):
    """Frames in 64-byte slots behind packed descriptors with the caller's flow ids; the restatement
    from the Python walk, and the host form bit for bit."""
    frames = [f for f, _ in slots]
    n = len(frames)
    data = np.frombuffer(b"".join(f + bytes(64 - len(f)) for f in frames), np.uint8)
    desc = (np.arange(n, dtype=np.uint64) * np.uint64(64)) | (np.array([m for _, m in slots], np.uint64) << np.uint64(48))
    ids = np.asarray(ids, np.uint32)
    src = Source(ctx, "edge", n, "packed", data=data, desc=desc)
    d_ids = upload(ctx, ids)
    try:
        facts = sr.facts_of_frames(frames)
        dirs = tr.directions(*fr.key_of_frames(frames, bool(flags & ftr.L3_ONLY)), flags)
        want = np.zeros(cap, sr.STAT_REC) if start is None else start.copy()
        want_res = sr.update(want, ids, facts, dirs, batch_ts if ts is None else ts)
        got = stat_call(ctx, src.batch, d_ids.ptr, flags, cap, want, want_res, ts=ts, batch_ts=batch_ts, start=start, where=where)
        host = np.zeros(cap, abi.FlowStatRec) if start is None else start.copy().view(abi.FlowStatRec)
        assert abi.flow_stat_update_host(data, desc, ids, flags, host, ts=ts, batch_ts=batch_ts) == want_res, where
        assert host.tobytes() == got, f"{where}: the host form"
        return want, want_res
    finally:
        src.free()
        d_ids.free()


@pytest.mark.parametrize("hi,lo", [(0, 16384), (63, 0), (16384, 63), (16383, 0)])
def test_one_flow_of_16385_packets_with_the_extremes_at_the_edges(gpu_ctx, hi, lo):
    """Every packet on one record, alternating direction: the sums wait in the waves, and after the
    first tiles the pre-read decides. Packet `hi` (and its neighbour of the other direction) carries
    the largest TTL, the shortest frame and the earliest stamps; packet `lo` (and its neighbour) the
    smallest TTL and the longest frame: at the first lane, the last lane of a tile and of a chunk,
    and the first packet of the second chunk."""
    n = 16385
    slots, ts = [], np.zeros(n, np.uint64)
    near = lambda i, p: i == p or i == (p + 1 if p % 2 == 0 and p + 1 < n else p - 1)  # noqa: E731
    for i in range(n):
        fl = (tr.SYN, tr.SYN | tr.ACK, tr.ACK, tr.ACK | tr.PSH)[(i // 2) % 4] if i % 2 == 0 else (tr.SYN | tr.ACK, tr.ACK, tr.SYN, tr.ACK)[(i // 2) % 4]
        ttl, length = (255, 54) if near(i, hi) else (2, 64) if near(i, lo) else (40 + i % 100, 56 + i % 7)
        ts[i] = 7 if near(i, hi) else 100000 + (i * 7919) % 50000
        slots.append(slot64(A, B, 1000, 80, fl, ttl, length, i % 50) if i % 2 == 0 else slot64(B, A, 80, 1000, fl, ttl, length, i % 3))
    if hi >= 8:   # every kind of stamp in both directions has its earliest time just below `hi`
        ts[hi - 8:hi] = 7
    want, res = crafted(gpu_ctx, slots, np.zeros(n, np.uint32), ftr.BIDIRECTIONAL, 1, f"one flow hi={hi} lo={lo}", ts=ts)
    d = abi.decode_flow_stat(want[0])
    assert res["tcp_packets"] == n and d["ttl_max"] == [255, 255] and d["ttl_min"] == [2, 2] and d["len_min"] == [54, 54] and d["len_max"] == [64, 64]
    assert 7 in d["syn_ts"] + d["synack_ts"] + d["ack_ts"] and None not in d["syn_ts"] + d["synack_ts"] + d["ack_ts"]
    # direction 0 is the 8193 even packets; their header says i % 50 bytes of payload: none for the 328 multiples of 50
    assert d["payload_packets"] == [8193 - 328, 8192 - 2731] and d["len_sq"][0] > 8192 * 54 * 54


def test_one_flow_onto_a_table_that_already_holds_more(gpu_ctx):
    """A non-zero starting table: the update adds to it and never resets it; the sums wrap."""
    n = 4097
    slots = [slot64(A, B, 1000, 80, tr.ACK, 40 + i % 9, 60, 5) if i % 2 == 0 else slot64(B, A, 80, 1000, tr.ACK, 50, 58, 0) for i in range(n)]
    start = np.zeros(2, sr.STAT_REC)
    start["seen"], start["proto_max"], start["ttl_max"], start["ttl_min_c"] = 0x01FF01FF, 200, [[255, 10]] * 2, [[U64_MAX & 0xFFFFFFFF, 5]] * 2
    start["len_max"], start["len_min_c"] = [[70, 1]] * 2, [[~np.uint32(10), 0]] * 2
    start["payload_packets"], start["payload_bytes"], start["len_sq"] = 0xFFFFFFF0, U64_MAX - 100, U64_MAX
    start["ack_ts_c"] = [[U64_MAX, 0]] * 2
    want, _ = crafted(gpu_ctx, slots, np.zeros(n, np.uint32), ftr.BIDIRECTIONAL, 2, "one flow, a full record", batch_ts=50, start=start)
    assert want[1].tobytes() == start[1].tobytes()
    assert int(want["payload_packets"][0, 0]) < 0xFFFFFFF0 and int(want["len_sq"][0, 0]) < U64_MAX and int(want["ttl_max"][0, 0]) == 255
    assert int(want["ack_ts_c"][0, 0]) == U64_MAX and int(want["ack_ts_c"][0, 1]) == U64_MAX - 50 and int(want["ttl_max"][0, 1]) == 50


def test_two_flows_interleaved(gpu_ctx):
    """A, B, A, B over 130 packets: the waiting sums are flushed whenever the other flow arrives."""
    slots = [slot64(A, B, 1000 + i % 2, 80, tr.ACK, 30 + i, 54 + i % 11, i) for i in range(130)]
    ids = np.arange(130, dtype=np.uint32) % 2
    want, res = crafted(gpu_ctx, slots, ids, 0, 2, "two flows", batch_ts=3)
    assert res["tcp_packets"] == 130 and int(want["payload_bytes"][0, 0]) == sum(range(0, 130, 2)) and int(want["payload_packets"][1, 0]) == 65
    want, _ = crafted(gpu_ctx, slots, 1 - ids, ftr.BIDIRECTIONAL, 2, "two flows, exchanged", ts=stamps(130, 1))
    assert int(want["payload_bytes"][1, 0]) == sum(range(0, 130, 2))


def test_64_distinct_flows_in_one_tile_and_ids_that_are_not_flows(gpu_ctx):
    slots = [slot64([10, 1, 0, k], B, 2000 + k, 443, (k * 5 + 2) & 255, 1 + k, 54 + k % 11, k) for k in range(64)]
    ids = np.arange(64, dtype=np.uint32)[::-1].copy()
    want, res = crafted(gpu_ctx, slots, ids, 0, 64, "64 flows", ts=stamps(64, 2))
    assert res["ip_packets"] == 64 and (want["ttl_max"][:, 0] != 0).all() and (want["len_sq"][:, 0] != 0).all()
    # flow numbers 256 apart share a byte of the wave's table of lone lanes: two lone flows per byte, then with a
    # second lane of flow 0 at the tile's end (three lanes on byte 0, two of them one flow)
    ids = np.concatenate([np.arange(32, dtype=np.uint32), 256 + np.arange(32, dtype=np.uint32)])
    want, res = crafted(gpu_ctx, slots, ids, ftr.BIDIRECTIONAL, 288, "flows 256 apart", ts=stamps(64, 3))
    assert res["ip_packets"] == 64 and int((want["len_sq"][:, 1] != 0).sum()) == 64
    ids[63] = 0
    want, _ = crafted(gpu_ctx, slots, ids, ftr.BIDIRECTIONAL, 288, "flows 256 apart and a pair", ts=stamps(64, 4))
    assert int(want["payload_bytes"][0, 1]) == 0 + 63 and int(want["payload_packets"][256, 1]) == 1 and not want["seen"][287]
    # sentinels contribute nothing and are not counted; 0xFFFFFFFC and ids at or past flow_cap are bad ids
    ids = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFB, 0xFFFFFFFC, 5, 6, 4] + [4] * 54, np.uint32)
    want, res = crafted(gpu_ctx, slots, ids, ftr.BIDIRECTIONAL, 5, "sentinels and bad ids", batch_ts=9)
    assert res["bad_ids"] == 3 and res["ip_packets"] == 57
    _, res = crafted(gpu_ctx, slots, np.arange(64, dtype=np.uint32), 0, 0, "flow_cap 0")
    assert res == {"n": 64, "ip_packets": 0, "l4_packets": 0, "tcp_packets": 0, "bad_ids": 64, "reserved": [0, 0, 0]}


@pytest.mark.parametrize("client,server", [(A, B), (B, A)])
def test_a_handshake_in_both_orientations_and_the_extreme_stamps(gpu_ctx, client, server):
    shake = [slot64(client, server, 5000, 80, tr.SYN), slot64(server, client, 80, 5000, tr.SYN | tr.ACK), slot64(client, server, 5000, 80, tr.ACK)]
    want, _ = crafted(gpu_ctx, shake, [0, 0, 0], ftr.BIDIRECTIONAL, 1, "handshake", ts=np.array([1000, 1030, 1075], np.uint64))
    d = int(client == B)
    got = abi.flow_stat_rtt(want[0])
    assert got == sr.rtt(want[0]) == {"has_initiator": 1, "initiator": d, "server_valid": 1, "client_valid": 1, "rtt_server": 30, "rtt_client": 45}
    # without BIDIRECTIONAL the answer never shares a record's direction 1: no RTT
    want, _ = crafted(gpu_ctx, shake, [0, 1, 0], 0, 2, "handshake, unidirectional", ts=np.array([1000, 1030, 1075], np.uint64))
    assert abi.flow_stat_rtt(want[0]) == {"has_initiator": 1, "initiator": 0, "server_valid": 0, "client_valid": 0, "rtt_server": 0, "rtt_client": 0}
    assert abi.flow_stat_rtt(want[1])["has_initiator"] == 0
    # stamps 0 and 2^64 - 2 are stamps; 2^64 - 1 reads as absent
    want, _ = crafted(gpu_ctx, shake + shake, [0] * 3 + [1] * 3, ftr.BIDIRECTIONAL, 2, "extreme stamps",
                      ts=np.array([0, U64_MAX - 1, U64_MAX - 1, U64_MAX, 5, 6], np.uint64))
    assert abi.flow_stat_rtt(want[0]) == {"has_initiator": 1, "initiator": d, "server_valid": 1, "client_valid": 1,
                                          "rtt_server": U64_MAX - 1, "rtt_client": 0}
    assert abi.flow_stat_rtt(want[1])["has_initiator"] == 0 and abi.decode_flow_stat(want[1])["synack_ts"][1 - d] == 5


def test_the_arithmetic_frames(gpu_ctx):
    """IPv6/TCP, QinQ/IPv4/UDP, ICMP, a fragment, IHL 6 and 4, the saturating cases and data offset 15
    (flowstat_cases.arithmetic_frames; test_flowstat.py holds the restatement to the numbers by hand)."""
    frames = [f for f, _ in arithmetic_frames()]
    data, desc = pack_frames(frames)
    n = len(frames)
    facts = sr.facts_of_frames(frames)
    ts = stamps(n, 5)
    for flags in ALL_FLAGS:
        dirs = tr.directions(*fr.key_of_frames(frames, bool(flags & ftr.L3_ONLY)), flags)
        for fmt, ids in (("packed", np.arange(n, dtype=np.uint32)), ("xdp", np.arange(n, dtype=np.uint32) % 3)):
            src = Source(gpu_ctx, "edge", n, fmt, data=data, desc=desc)
            d_ids = upload(gpu_ctx, ids)
            try:
                want = np.zeros(n, sr.STAT_REC)
                want_res = sr.update(want, ids, facts, dirs, ts)
                got = stat_call(gpu_ctx, src.batch, d_ids.ptr, flags, n, want, want_res, ts=ts, where=f"arithmetic {fmt} flags={flags}")
                host = np.zeros(n, abi.FlowStatRec)
                assert abi.flow_stat_update_host(data, desc, ids, flags, host, ts=ts) == want_res and host.tobytes() == got
            finally:
                src.free()
                d_ids.free()
    assert want_res["ip_packets"] == 17 and want_res["l4_packets"] == 12 and want_res["tcp_packets"] == 10


def test_bytes_cutting_the_last_frame_at_every_header_offset(gpu_ctx):
    """An IPv4 / TCP frame with 100 bytes of payload, placed so that the cut falls on a 16-byte
    boundary of the (16-byte aligned) buffer: the fan-out's read rule then cuts exactly at `bytes`,
    as the host form does. Cut at every offset of the IP and TCP headers and behind them: the
    missing bytes read as zero, the frame keeps its length."""
    frame = ip4(6, tcp_hdr(1000, 80, tr.SYN | tr.ACK, doff=6) + bytes(104), B, A, ttl=77)
    whole = sr.facts_of_frames([frame])
    assert whole["payload"][0] == 100 and whole["stamp"][0] == sr.SYNACK_STAMP
    seen_payload = set()
    for cut in range(14, 14 + 40 + 2):
        off = 32 - cut % 16 if cut % 16 else 32
        nbytes = off + cut
        assert nbytes % 16 == 0
        data = np.full(off + len(frame) + 16, 0xEE, np.uint8)   # what lies past `bytes` is not zero: it must not be read
        data[off:off + len(frame)] = np.frombuffer(frame, np.uint8)
        desc = np.array([off | len(frame) << 48], np.uint64)
        seen = frame[:cut] + bytes(len(frame) - cut)
        facts = sr.facts_of_frames([seen])
        dirs = tr.directions(*fr.key_of_frames([seen]), ftr.BIDIRECTIONAL)
        src = Source(gpu_ctx, "edge", 1, "packed", data=data, desc=desc, nbytes=nbytes)
        d_ids = upload(gpu_ctx, np.zeros(1, np.uint32))
        try:
            assert src.d_data.ptr % 16 == 0
            want = np.zeros(1, sr.STAT_REC)
            want_res = sr.update(want, [0], facts, dirs, 11)
            got = stat_call(gpu_ctx, src.batch, d_ids.ptr, ftr.BIDIRECTIONAL, 1, want, want_res, batch_ts=11, where=f"cut={cut}")
            host = np.zeros(1, abi.FlowStatRec)
            assert abi.flow_stat_update_host(data, desc, [0], ftr.BIDIRECTIONAL, host, batch_ts=11, nbytes=nbytes) == want_res
            assert host.tobytes() == got, f"cut={cut}: the host form"
            seen_payload.add(int(want["payload_bytes"][0].sum()))
        finally:
            src.free()
            d_ids.free()
    assert facts["payload"][0] == 100 and {0, 124, 100} <= seen_payload   # no protocol byte; no data offset byte: 144 - 20 - 0; whole


class DevStatTracker:
    """A tracker, its statistics side table and two more side tables (4-byte and TCP records) on the
    device, with the restatement beside them. Every call is prepared first, then all of them are
    enqueued back to back and waited for once."""

    def __init__(self, ctx, flow_cap, flags):
        self.ctx, self.cap, self.flags = ctx, flow_cap, flags
        self.layout = abi.flow_track_layout(flow_cap)
        self.state, self.stat = Guarded(ctx, self.layout["total"]), Guarded(ctx, REC * flow_cap)
        abi._check(abi.lib().bt_memset_d(ctx.h, self.stat.ptr, 0, REC * flow_cap))
        self.ref, self.want = fkr.Tracker(flow_cap, flags), np.zeros(flow_cap, sr.STAT_REC)
        self.calls, self.checks, self.bufs = [], [], []

    def update(self, src, keys, facts, dirs, ts, batch_ts, where):
        ctx, n = self.ctx, src.n
        need = abi.flow_track_scratch_bytes(n)
        ids, res, scratch, sres = Guarded(ctx, 4 * n), Guarded(ctx, 64), Guarded(ctx, need), Guarded(ctx, 32)
        d_ts = upload(ctx, ts) if ts is not None else None
        self.bufs += [ids, res, scratch, sres] + ([d_ts] if d_ts is not None else [])
        want_ids = self.ref.update(keys[0], keys[1], keys[2], src.lens, None, ts, batch_ts)["flow_id"]
        want_res = sr.update(self.want, want_ids, facts, dirs, batch_ts if ts is None else ts)

        def call():
            ctx.flow_track_update(self.state.ptr, src.batch, scratch.ptr, need, res.ptr, ts=d_ts, batch_ts=batch_ts, flow_id=ids.ptr)
            ctx.flow_stat_update(src.batch, ids.ptr, self.flags, self.stat.ptr, self.cap, sres.ptr, ts=d_ts, batch_ts=batch_ts)

        def check():
            assert (ids.read(np.uint32) == want_ids).all(), f"{where}: flow ids"
            assert abi.FlowStatResult.from_bytes(sres.read()).as_dict() == want_res, f"{where}: result"
        self.calls.append(call)
        self.checks.append(check)
        return want_ids

    def expire_and_move(self, now, idle, expired_cap, where):
        ctx, cap = self.ctx, self.cap
        need, mneed = abi.flow_track_expire_scratch_bytes(cap), abi.flow_track_side_move_scratch_bytes(cap, REC)
        exp, gone, remap = Guarded(ctx, 104 * expired_cap), Guarded(ctx, REC * expired_cap), Guarded(ctx, 4 * cap)
        res, scratch, mscratch = Guarded(ctx, 32), Guarded(ctx, need), Guarded(ctx, mneed)
        self.bufs += [exp, gone, remap, res, scratch, mscratch]
        before = len(self.ref.flows)
        want = self.ref.expire(now, idle, expired_cap)
        want_gone = sr.side_move(self.want, want["remap"], want["result"], expired_cap)

        def call():
            ctx.flow_track_expire(self.state.ptr, now, idle, scratch.ptr, need, res.ptr, expired=exp.ptr, expired_cap=expired_cap,
                                  remap=remap.ptr)
            ctx.flow_track_side_move(self.stat.ptr, REC, cap, remap.ptr, res.ptr, mscratch.ptr, mneed, expired_side=gone.ptr,
                                     expired_cap=expired_cap)
        out = {}

        def check():
            got = abi.FlowTrackExpireResult.from_bytes(res.read()).as_dict()
            assert got == want["result"] and got["n_flows_before"] == before, f"{where}: expire result {got}"
            ne = got["n_expired"]
            assert (remap.read(np.uint32)[:before] == want["remap"]).all(), f"{where}: remap"
            g = gone.read()
            assert g[:REC * ne].tobytes() == want_gone.tobytes() and (g[REC * ne:] == POISON).all(), f"{where}: the expired flows' statistics"
            mscratch.read()
            out.update(result=got, gone=want_gone)
        self.calls.append(call)
        self.checks.append(check)
        return out

    def finish(self):
        ctx = self.ctx
        ctx.synchronize()
        ctx.flow_track_init(self.state.ptr, self.layout["total"], self.cap, self.flags)
        for call in self.calls:
            call()
        ctx.synchronize()
        for check in self.checks:
            check()
        table = self.stat.read()
        assert table.tobytes() == self.want.tobytes(), "the side table"
        return table.tobytes()

    def free(self):
        abi.Context.flow_track_forget(self.state.ptr)
        for b in self.bufs + [self.state, self.stat]:
            b.free()


def tracked(ctx, name, flags, cap, batches, expire_at):
    """Batches of a golden through a tracker with a small flow_cap (an overflow), the statistics
    behind each, one expire with the side move in between. Batch b is stamped 10 b, or per packet
    10 b .. 10 b + 4 on the odd batches."""
    g, _ = load_golden(name)
    n0 = len(g["desc"])
    keys = golden_keys(name, bool(flags & ftr.L3_ONLY))
    facts, dirs = packet_facts(name, False), packet_dirs(name, False, flags)
    t = DevStatTracker(ctx, cap, flags)
    srcs, out = [], None
    try:
        for b, (n, start) in enumerate(batches):
            if b == expire_at:
                out = t.expire_and_move(10 * b, 15, cap, f"{name} expire")
            reps = (start + np.arange(n)) % n0
            src = Source(ctx, name, n, "packed", desc=g["desc"][reps])
            srcs.append(src)
            ts = (np.uint64(10 * b) + (np.arange(n) % 5).astype(np.uint64)) if b % 2 else None
            ids = t.update(src, (keys[0][reps], keys[1][reps], keys[2][reps]), facts[reps], dirs[reps], ts, 10 * b, f"{name} batch {b}")
        return t.finish(), out, t.ref, ids
    finally:
        t.free()
        for s in srcs:
            s.free()


BATCHES = [(700, 0), (65, 650), (16385, 300), (64, 0)]


@pytest.mark.parametrize("name,flags,cap", [("c4", ftr.BIDIRECTIONAL, 900), ("fuzz", 0, 400), ("c3", ftr.L3_ONLY | ftr.BIDIRECTIONAL, 4096)])
def test_ids_from_a_tracker_with_an_overflow_and_an_expire_in_between(gpu_ctx, name, flags, cap):
    table, out, ref, ids = tracked(gpu_ctx, name, flags, cap, BATCHES, 2)
    again = tracked(gpu_ctx, name, flags, cap, BATCHES, 2)
    assert table == again[0]   # two runs byte-equal
    r = out["result"]
    assert r["n_expired"] > 0 and r["n_flows"] > 0 and out["gone"]["len_sq"].any()
    if cap < 4096:
        assert ref.header()["overflow_packets"] > 0 and (ids == abi.FLOW_ID_OVERFLOW).any()


def conversations(nflows, batch):
    """One TCP packet for each of nflows conversations (batch 0), or for every third one from the second on (batch 1)."""
    ks = range(nflows) if batch == 0 else range(1, nflows, 3)
    return [slot64([10, 2, k >> 8, k & 255], B, 3000, 80, (tr.SYN, tr.ACK | tr.FIN, tr.RST)[k % 3], 9 + k % 200, 54 + k % 11, k % 40) for k in ks]


@pytest.mark.parametrize("cap", [1, 255, 256, 257])
def test_the_generic_move_against_the_tcp_expire_and_the_restatement(gpu_ctx, cap):
    """Two identical trackers of flow_cap flows, all of them live; a third of them seen again later.
    On one, bt_flow_track_expire_tcp_device with closed_idle = 2^64 - 1 carries the TCP side table
    itself. On the other the plain expire runs, and the generic move carries a TCP side table
    (rec_bytes 16), a table of 4-byte records and the statistics (128) by its remap: tcp[] and
    expired_tcp[] must be byte-equal to the first tracker's, the others equal the restatement. The
    expire's expired_cap is below the idle flows (but for flow_cap 1), the 4-byte move's lower still."""
    ctx = gpu_ctx
    xcap = 1 if cap == 1 else 40
    lay = abi.flow_track_layout(cap)
    frames0, frames1 = conversations(cap, 0), conversations(cap, 1)
    ref, stat_want, word_want = fkr.Tracker(cap, 0), np.zeros(cap, sr.STAT_REC), np.arange(1, cap + 1, dtype=np.uint32)
    bufs, runs = [], []
    try:
        for which in ("tcp", "generic"):
            state, tcp, stat, word = Guarded(ctx, lay["total"]), Guarded(ctx, 16 * cap), Guarded(ctx, REC * cap), Guarded(ctx, 4 * cap)
            exp, exp_tcp, exp_stat, exp_word = Guarded(ctx, 104 * xcap), Guarded(ctx, 16 * xcap), Guarded(ctx, REC * xcap), Guarded(ctx, 4 * xcap)
            remap, xres = Guarded(ctx, 4 * cap), Guarded(ctx, 32)
            need = abi.flow_track_expire_tcp_scratch_bytes(cap)
            xscratch = Guarded(ctx, need)
            mneed = [abi.flow_track_side_move_scratch_bytes(cap, rb) for rb in (16, REC, 4)]
            mscratch = [Guarded(ctx, m) for m in mneed]
            bufs += [state, tcp, stat, word, exp, exp_tcp, exp_stat, exp_word, remap, xres, xscratch] + mscratch
            abi._check(abi.lib().bt_memset_d(ctx.h, tcp.ptr, 0, 16 * cap))
            abi._check(abi.lib().bt_memset_d(ctx.h, stat.ptr, 0, REC * cap))
            abi._check(abi.lib().bt_memcpy_h2d(ctx.h, word.ptr, word_want.ctypes.data, 4 * cap))
            ctx.synchronize()
            ctx.flow_track_init(state.ptr, lay["total"], cap, 0)
            for b, slots in enumerate((frames0, frames1)):
                if not slots:   # flow_cap 1: nobody is seen again
                    continue
                frames = [f for f, _ in slots]
                n = len(frames)
                data = np.frombuffer(b"".join(f + bytes(64 - len(f)) for f in frames), np.uint8)
                desc = (np.arange(n, dtype=np.uint64) * np.uint64(64)) | (np.array([m for _, m in slots], np.uint64) << np.uint64(48))
                src = Source(ctx, "edge", n, "packed", data=data, desc=desc)
                ids, res, scratch, sres = Guarded(ctx, 4 * n), Guarded(ctx, 64), Guarded(ctx, abi.flow_track_scratch_bytes(n)), Guarded(ctx, 32)
                bufs += [src, ids, res, scratch, sres]
                ctx.flow_track_update(state.ptr, src.batch, scratch.ptr, scratch.size, res.ptr, batch_ts=100 * b, flow_id=ids.ptr)
                ctx.flow_tcp_update(src.batch, ids.ptr, 0, tcp.ptr, cap, sres.ptr)
                ctx.flow_stat_update(src.batch, ids.ptr, 0, stat.ptr, cap, sres.ptr, batch_ts=100 * b)
                if which == "generic":   # the restatement, once
                    keys = fr.key_of_frames(frames)
                    wid = ref.update(*keys, np.array([m for _, m in slots], np.int64), None, None, 100 * b)["flow_id"]
                    sr.update(stat_want, wid, sr.facts_of_frames(frames), np.zeros(n, np.int64), 100 * b)
            if which == "tcp":
                ctx.flow_track_expire_tcp(state.ptr, 100, 50, U64_MAX, tcp.ptr, xscratch.ptr, need, xres.ptr, expired=exp.ptr,
                                          expired_cap=xcap, expired_tcp=exp_tcp.ptr, remap=remap.ptr)
            else:
                pneed = abi.flow_track_expire_scratch_bytes(cap)
                ctx.flow_track_expire(state.ptr, 100, 50, xscratch.ptr, pneed, xres.ptr, expired=exp.ptr, expired_cap=xcap, remap=remap.ptr)
                ctx.flow_track_side_move(tcp.ptr, 16, cap, remap.ptr, xres.ptr, mscratch[0].ptr, mneed[0], expired_side=exp_tcp.ptr,
                                         expired_cap=xcap)
                ctx.flow_track_side_move(stat.ptr, REC, cap, remap.ptr, xres.ptr, mscratch[1].ptr, mneed[1], expired_side=exp_stat.ptr,
                                         expired_cap=xcap)
                ctx.flow_track_side_move(word.ptr, 4, cap, remap.ptr, xres.ptr, mscratch[2].ptr, mneed[2], expired_side=exp_word.ptr,
                                         expired_cap=max(1, xcap - 9))
            ctx.synchronize()
            for m in mscratch:
                m.read()
            runs.append({"state": state.read().tobytes()[:lay["slot_words"]], "tcp": tcp.read().tobytes(), "exp_tcp": exp_tcp.read().tobytes(),
                         "remap": remap.read(np.uint32), "res": abi.FlowTrackExpireResult.from_bytes(xres.read()).as_dict(),
                         "stat": stat.read().tobytes(), "exp_stat": exp_stat.read(), "word": word.read(np.uint32), "exp_word": exp_word.read(np.uint32)})
            abi.Context.flow_track_forget(state.ptr)
        a, b = runs
        r = b["res"]
        idle = cap - len(range(1, cap, 3))
        assert a["res"] == r and r["n_flows_before"] == cap and r["n_idle"] == idle and r["n_expired"] == min(idle, xcap) and r["status"] == 0
        assert (a["remap"] == b["remap"]).all() and a["state"] == b["state"]
        assert a["tcp"] == b["tcp"], "tcp[] moved by the generic move differs from the TCP-aware expire's"
        assert a["exp_tcp"] == b["exp_tcp"], "expired_tcp[]"
        if cap > 1:
            assert r["n_idle"] > xcap and any(a["tcp"])
        # the statistics and the 4-byte records against the restatement
        want = ref.expire(100, 50, xcap)
        assert want["result"] == r and (want["remap"] == b["remap"][:cap]).all()
        gone = sr.side_move(stat_want, want["remap"], r, xcap)
        assert b["stat"] == stat_want.tobytes() and b["exp_stat"][:REC * len(gone)].tobytes() == gone.tobytes()
        assert (b["exp_stat"][REC * len(gone):] == POISON).all()
        wgone = sr.side_move(word_want, want["remap"], r, max(1, xcap - 9))
        assert (b["word"] == word_want).all() and (b["exp_word"][:len(wgone)] == wgone).all()
        assert (b["exp_word"][len(wgone):] == np.uint32(0x01010101 * POISON)).all() and len(wgone) == min(r["n_expired"], max(1, xcap - 9))
    finally:
        for x in bufs:
            x.free()


def test_an_expire_that_refuses_the_state_moves_nothing(gpu_ctx):
    """The header overwritten behind the library's back: the expire reports status 1 with every count
    0 and leaves remap alone; the move behind it writes nothing. So does a move behind an expire
    that found no idle flow."""
    ctx, cap = gpu_ctx, 300
    lay = abi.flow_track_layout(cap)
    state, side, gone, remap, xres = Guarded(ctx, lay["total"]), Guarded(ctx, REC * cap), Guarded(ctx, REC * 8), Guarded(ctx, 4 * cap), Guarded(ctx, 32)
    need, mneed = abi.flow_track_expire_scratch_bytes(cap), abi.flow_track_side_move_scratch_bytes(cap, REC)
    xscratch, mscratch = Guarded(ctx, need), Guarded(ctx, mneed)
    slots = conversations(200, 0)
    frames = [f for f, _ in slots]
    data = np.frombuffer(b"".join(f + bytes(64 - len(f)) for f in frames), np.uint8)
    src = Source(ctx, "edge", 200, "packed", data=data, desc=np.arange(200, dtype=np.uint64) * np.uint64(64) | np.uint64(64 << 48))
    res, scratch = Guarded(ctx, 64), Guarded(ctx, abi.flow_track_scratch_bytes(200))
    try:
        fill = np.arange(REC * cap // 4, dtype=np.uint32)
        abi._check(abi.lib().bt_memcpy_h2d(ctx.h, side.ptr, fill.ctypes.data, REC * cap))
        ctx.synchronize()
        ctx.flow_track_init(state.ptr, lay["total"], cap, 0)
        ctx.flow_track_update(state.ptr, src.batch, scratch.ptr, scratch.size, res.ptr, batch_ts=5)
        ctx.flow_track_expire(state.ptr, 6, 100, xscratch.ptr, need, xres.ptr, expired=None, remap=remap.ptr)   # nobody is idle
        ctx.flow_track_side_move(side.ptr, REC, cap, remap.ptr, xres.ptr, mscratch.ptr, mneed, expired_side=gone.ptr, expired_cap=8)
        ctx.synchronize()
        x = abi.FlowTrackExpireResult.from_bytes(xres.read()).as_dict()
        assert (x["n_flows_before"], x["n_flows"], x["n_expired"], x["status"]) == (200, 200, 0, 0)
        assert (side.read(np.uint32) == fill).all() and (gone.read() == POISON).all()
        abi._check(abi.lib().bt_memset_d(ctx.h, state.ptr, 0, 128))
        abi._check(abi.lib().bt_memset_d(ctx.h, remap.buf.ptr, POISON, remap.buf.nbytes))
        ctx.flow_track_expire(state.ptr, 1000, 1, xscratch.ptr, need, xres.ptr, expired=None, remap=remap.ptr)
        ctx.flow_track_side_move(side.ptr, REC, cap, remap.ptr, xres.ptr, mscratch.ptr, mneed, expired_side=gone.ptr, expired_cap=8)
        ctx.synchronize()
        x = abi.FlowTrackExpireResult.from_bytes(xres.read()).as_dict()
        assert x == {**dict.fromkeys(x, 0), "status": 1, "reserved": [0, 0, 0]}
        assert (side.read(np.uint32) == fill).all() and (gone.read() == POISON).all() and (remap.read() == POISON).all()
        mscratch.read()
    finally:
        abi.Context.flow_track_forget(state.ptr)
        for b in (state, side, gone, remap, xres, xscratch, mscratch, src, res, scratch):
            b.free()
